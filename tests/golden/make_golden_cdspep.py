"""Record what the REFERENCE's own get_CDS_peptides writes:
tests/golden/get_cds_peptides.json.

Runs only where the reference is installed (see make_golden.py, whose lib2to3
copy this imports); nothing of the reference's program text is stored, only
inputs, outputs, hashes and exception names.

The reference's get_CDS_peptides (genome_tools.py:283-321) calls
``Genome.read_gff3``, which does not exist.  Here its ``Genome``
is subclassed to give it ``read_gff3 = read_gff``; the function body itself
runs unchanged.

The copy runs under Python 3, so ``annotations.gene`` iterates in insertion
order: every record is the ``order='insertion'`` output.  The Python 2 order of
the same dict is the one tests/golden/fixtures.json pins for gff2fasta
(oracle.magot_oracle.py2_order_after_deepcopy).

Per case (tests/cdspep_expect.py TOOL_CASES): ``kw`` (the keyword arguments),
``fasta_sha`` / ``gff_sha`` of the inputs, ``exc`` (exception name or null),
``file`` (whether the run opened its output file at all), ``sha`` and ``size``
of what the run wrote, ``out`` in full when short, and
``stdout``.

Usage:  python tests/golden/make_golden_cdspep.py
"""

import builtins
import gc
import json
import os
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))

import make_golden  # noqa: E402
import cdspep_expect as ce  # noqa: E402
import orfs_expect as oe  # noqa: E402

KEEP_TEXT = 4096


def reference_tools():
    ref = make_golden.reference_module()
    import genome_tools as tools
    import magot_smallfuncs as small
    small.open = lambda path, *a, **k: builtins.open(path, newline='\n', encoding='latin-1')
    original = ref.Genome

    class Gff3Genome(original):
        read_gff3 = original.read_gff

    tools.genome.Genome = Gff3Genome
    return tools


def main():
    tools = reference_tools()
    cases = {}
    with tempfile.TemporaryDirectory() as tmp:
        fa, gff, out = (os.path.join(tmp, n) for n in ('in.fa', 'in.gff', 'out.fa'))
        for name in ce.TOOL_CASES:
            fasta_text, gff_text, kw = ce.tool_inputs(name, HERE)
            for path, text in ((fa, fasta_text), (gff, gff_text)):
                with open(path, 'w', encoding='latin-1', newline='') as fh:
                    fh.write(text)
            if os.path.exists(out):
                os.remove(out)
            _, exc, printed = make_golden.call(lambda: tools.get_CDS_peptides(fa, gff, out, **kw))
            gc.collect()  # the reference leaves its file to the collector
            text = ''
            if os.path.exists(out):  # not opened where read_gff3 itself raises
                with open(out, encoding='latin-1', newline='') as fh:
                    text = fh.read()
            case = {'kw': kw, 'file': os.path.exists(out), 'fasta_sha': oe.sha(fasta_text), 'gff_sha': oe.sha(gff_text),
                    'exc': exc, 'sha': oe.sha(text), 'size': len(text), 'stdout': printed}
            if len(text) <= KEEP_TEXT:
                case['out'] = text
            cases[name] = case
            print(name, exc, len(text), flush=True)
    with open(os.path.join(HERE, 'get_cds_peptides.json'), 'w') as fh:
        json.dump({'cases': cases}, fh, indent=0, sort_keys=True)
        fh.write('\n')


if __name__ == '__main__':
    main()
