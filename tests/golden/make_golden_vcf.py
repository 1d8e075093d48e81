"""Record what the REFERENCE's own read_vcf and calculate_heterozygosity give:
tests/golden/vcf.json.

Runs only where the reference is installed (see make_golden.py, whose lib2to3
copy this imports); the two reference functions (magot_variants.py:16-139) run
unchanged, and nothing of their program text is stored: only inputs, stdout,
returned strings, exception names and each case's note of its path.

The copy runs under Python 3, which differs from the Python 2 target in the
places below; all are handled here, not in the copy, by substituting names in
the imported modules:

  * ``open`` (magot_smallfuncs, whose read_to_string reads the file): text mode
    would translate line ends and decode UTF-8.  The shadow opens with
    ``newline='\\n'`` and ``encoding='latin-1'``; read_to_string then drops every
    CR itself, as it does under Python 2.
  * ``str``: the Python 2 rule for a float (twelve significant digits), the
    builtin for everything else.
  * ``int``: the Python 2 reading (no ``_``, ASCII digits).
  * ``set`` and ``list``: ``list(set(loci))``, ``list(variant_set)`` and
    ``list(counts_of_a_locus)`` follow CPython 2.7's slot order.  ``set`` becomes
    a list that remembers the order its items came in; ``list`` of it, and of a
    dict, gives the keys in the order oracle.magot_oracle.py2_dict_order derives
    from their insertion order: for the VariantSet as inserted, for the counts
    of a locus after two rebuilds (the genotypes dict was deep-copied once and
    then re-inserted into the counts).  For the 'insertion' record both give the
    distinct keys as first seen.  The list of names prints with Python 2's repr
    of byte strings.
  * ``seqlen / window``: ``window`` is passed as an int subclass whose
    ``__rtruediv__`` floors, which Python tries before int's own true division.

The set order rests on Python 2.7's set using the dict's slot model: the same
probe sequence, the same growth rule (setobject.c's set_add_entry and
set_table_resize against dictobject.c).  No Python 2 is at hand where this runs
to confirm it by execution.

Per case: ``text`` (the file's bytes as latin-1), ``loci`` (null: from the
header), ``window``, and per order ('py2', 'insertion') ``out``, ``ret``, ``exc``
and ``note`` ('native', 'raise' -- the device path raises the KeyError itself --
or the reason the device path declines for; vcf_expect.native_note).

Usage:  python tests/golden/make_golden_vcf.py
"""

import builtins
import json
import os
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

import make_golden  # noqa: E402
import vcf_expect as ve  # noqa: E402
from oracle import magot_oracle as mo  # noqa: E402


class FloorWindow(int):
    def __rtruediv__(self, other):
        return other // int(self)


class SeenOrder(builtins.list):
    """what set() returns here: the items in the order they came"""


class Py2Names(builtins.list):
    def __repr__(self):
        return '[' + ', '.join(ve.py2_repr(x) if isinstance(x, builtins.str) else repr(x)
                               for x in self) + ']'


def shadow(variants, smallfuncs, order):
    def py2_list(value=()):
        if isinstance(value, SeenOrder):
            keys = builtins.list(dict.fromkeys(value))
            return mo.py2_dict_order(keys) if order == 'py2' else keys
        if isinstance(value, dict):
            keys = builtins.list(value)
            if order == 'py2':
                keys = mo.py2_dict_order(keys)
                if type(value) is dict:  # the counts of a locus
                    keys = mo.py2_dict_order(mo.py2_dict_order(keys))
            return Py2Names(keys)
        return builtins.list(value)

    smallfuncs.open = lambda path, *a, **k: builtins.open(path, newline='\n', encoding='latin-1')
    variants.str = lambda v: ve.py2_float_str(v) if isinstance(v, float) else builtins.str(v)
    variants.int = ve.py2_int
    variants.set = SeenOrder
    variants.list = py2_list


def main():
    make_golden.reference_module()
    import magot_smallfuncs as smallfuncs
    import magot_variants as variants
    gold = {}
    with tempfile.TemporaryDirectory() as tmp:
        path = os.path.join(tmp, 'calls.vcf')
        for name, (text, loci, window) in ve.cases().items():
            with open(path, 'wb') as fh:
                fh.write(text.encode('latin-1'))
            rec = {'text': text, 'loci': loci, 'window': window}
            for order in ve.ORDERS:
                shadow(variants, smallfuncs, order)
                ret, exc, out = make_golden.call(lambda: variants.calculate_heterozygosity(
                    variants.read_vcf(path), None if loci is None else builtins.list(loci),
                    FloorWindow(window)))
                rec[order] = {'out': out, 'ret': ret, 'exc': exc,
                              'note': ve.native_note(text, loci, window, order)}
            gold[name] = rec
            print(name, [(rec[o]['exc'], rec[o]['note']) for o in ve.ORDERS], flush=True)
    with open(os.path.join(HERE, 'vcf.json'), 'w') as fh:
        json.dump(gold, fh, indent=0, sort_keys=True)
        fh.write('\n')


if __name__ == '__main__':
    main()
