"""Record what the REFERENCE's own composition_by_site prints:
tests/golden/site.json.

Runs only where the reference is installed (see make_golden.py, whose
lib2to3 copy this imports); the reference function (genome_tools.py:488-503)
runs unchanged, and nothing of its program text is stored: only inputs, stdout,
exception names and the case's note of its path.

The copy runs under Python 3, which differs from the Python 2 target in two
places this function touches; both are handled here, not in the copy, by
substituting a name in the copied module:

  * ``str``: Python 3 prints a float's shortest repr, Python 2 twelve
    significant digits.  The shadow is the Python 2 rule for a float
    (site_expect.py2_float_str) and the builtin for everything else.
  * ``list``, for the ``out_py2`` record only: the number of sites is the
    length of ``list(seq_dict)[0]``, the dict's first key -- first inserted
    under Python 3, first in slot order under Python 2.  The shadow returns a
    dict's keys in the order oracle.magot_oracle.py2_dict_order gives them.
    The loops over the records themselves add and compare, so their order
    does not show.

Per case: ``text`` (the file's bytes as latin-1; null for the generated tall
case, ``gen`` naming its generator in site_expect), ``out`` and ``exc`` (stdout
and exception name with the first key by insertion), ``out_py2`` and ``exc_py2``
(by Python 2's order) and ``note`` ('native', or why the device path must raise
or decline).

Usage:  python tests/golden/make_golden_site.py
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
import site_expect as se  # noqa: E402
from oracle import magot_oracle as mo  # noqa: E402


def py2_str(value):
    return se.py2_float_str(value) if isinstance(value, float) else builtins.str(value)


def py2_list(value=()):
    if isinstance(value, dict):
        return mo.py2_dict_order(builtins.list(value))
    return builtins.list(value)


def main():
    make_golden.reference_module()
    import genome_tools as tools
    tools.str = py2_str
    gold = {}
    with tempfile.TemporaryDirectory() as tmp:
        path = os.path.join(tmp, 'aln.fa')
        for name, (text, note) in se.cases().items():
            rec = {'text': None if text is None else text.decode('latin-1'), 'note': note}
            if text is None:
                rec['gen'] = name
                text = se.text_of(rec)
            with open(path, 'wb') as fh:
                fh.write(text)
            tools.list = builtins.list
            _, rec['exc'], rec['out'] = make_golden.call(lambda: tools.composition_by_site(path))
            tools.list = py2_list
            _, rec['exc_py2'], rec['out_py2'] = make_golden.call(
                lambda: tools.composition_by_site(path))
            gold[name] = rec
            print(name, rec['exc'], rec['exc_py2'], note, len(rec['out']), flush=True)
    with open(os.path.join(HERE, 'site.json'), 'w') as fh:
        json.dump(gold, fh, indent=0, sort_keys=True)
        fh.write('\n')


if __name__ == '__main__':
    main()
