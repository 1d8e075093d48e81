"""Record what the REFERENCE's own dna2orfs writes: tests/golden/dna2orfs.json.

Runs only where the reference is installed (see make_golden.py, whose
lib2to3 copy this imports); nothing of the reference's program text is
stored, only inputs, outputs, hashes and exception names.

The reference's dna2orfs (genome_tools.py:145-180) hands ``translate`` the
plain ``str`` values of GenomeSequence and dies with a TypeError on its first
contig.  Here its ``Genome`` is subclassed to wrap every
contig in the reference's own ``Sequence``, which is what the rest of the
function assumes; the function body itself runs unchanged.

Per case (inputs from tests/orfs_expect.py, plus the shipped O.biroi subset)
and per (from_atg, longest) mode:
  exc      exception name of the whole-file run, or null
  sha      sha256 of what that run wrote (Python 3: insertion order)
  text     the same in full when short
  blocks   sha256 of what a run over each contig alone wrote, in input order
           (their concatenation up to the first failure is the whole-file
           output: asserted here)
  sha_py2  sha256 of the blocks in CPython 2.7 dict order
           (oracle.magot_oracle.py2_dict_order), up to the first failure

Usage:  python tests/golden/make_golden_orfs.py
"""

import gc
import json
import os
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
TESTS = os.path.dirname(HERE)
sys.path.insert(0, TESTS)
sys.path.insert(0, HERE)

import make_golden  # noqa: E402
from make_golden import mo  # noqa: E402
import orfs_expect as oe  # noqa: E402

OBIROI = 'O.biroi_refseqGenomeSubset.fasta'
KEEP_TEXT = 2048
KEEP_INPUT = 4096


def reference_tools():
    ref = make_golden.reference_module()
    import genome_tools as tools
    original = ref.Genome  # patching the name the subclass inherits from would recurse

    class SequenceGenome(original):
        def __init__(self, *args, **kw):
            original.__init__(self, *args, **kw)
            for name in list(self.genome_sequence):
                self.genome_sequence[name] = ref.Sequence(self.genome_sequence[name])

    tools.genome.Genome = SequenceGenome
    return tools


def run(tools, fasta_text, from_atg, longest, tmp):
    """(what the reference wrote, exception name or None)."""
    fa = os.path.join(tmp, 'in.fa')
    out = os.path.join(tmp, 'out.fa')
    with open(fa, 'w', encoding='latin-1', newline='') as fh:
        fh.write(fasta_text)
    if os.path.exists(out):
        os.remove(out)
    exc = None
    try:
        tools.dna2orfs(fa, out, from_atg=from_atg, longest=longest)
    except Exception as e:  # noqa: BLE001
        exc = type(e).__name__
    gc.collect()  # the reference leaves its file to the collector on a failure
    with open(out, encoding='latin-1', newline='') as fh:
        return fh.read(), exc


def record(tools, contigs, fasta_text, tmp):
    seqs = dict(contigs)
    names = list(seqs)
    modes = {}
    for from_atg, longest in oe.MODES:
        text, exc = run(tools, fasta_text, from_atg, longest, tmp)
        blocks = [run(tools, oe.fasta([(nm, seqs[nm])]), from_atg, longest, tmp) for nm in names]
        by_name = dict(zip(names, blocks))

        def joined(order):
            parts = []
            for nm in order:
                parts.append(by_name[nm][0])
                if by_name[nm][1]:
                    return ''.join(parts), by_name[nm][1]
            return ''.join(parts), None

        assert joined(names) == (text, exc), (from_atg, longest)
        entry = {'exc': exc, 'sha': oe.sha(text), 'blocks': [oe.sha(b[0]) for b in blocks],
                 'sha_py2': oe.sha(joined(mo.py2_dict_order(names))[0]),
                 'exc_py2': joined(mo.py2_dict_order(names))[1]}
        if len(text) <= KEEP_TEXT:
            entry['text'] = text
        modes['%d%d' % (from_atg, longest)] = entry
    return modes


def main():
    tools = reference_tools()
    cases = {}
    with tempfile.TemporaryDirectory() as tmp:
        for name, make in oe.CASES.items():
            contigs = make()
            text = oe.fasta(contigs)
            case = {'input_sha': oe.sha(text), 'modes': record(tools, contigs, text, tmp)}
            if len(text) <= KEEP_INPUT:
                case['input'] = text
            cases[name] = case
            print(name, {m: e['exc'] for m, e in case['modes'].items()}, flush=True)
        with open(os.path.join(HERE, OBIROI), encoding='latin-1', newline='') as fh:
            text = fh.read()
        contigs = mo.read_fasta(os.path.join(HERE, OBIROI))
        contigs = list(contigs.items()) if hasattr(contigs, 'items') else list(contigs)
        cases['obiroi'] = {'input_file': OBIROI, 'input_sha': oe.sha(text),
                           'modes': record(tools, contigs, text, tmp)}
        print('obiroi', len(contigs), flush=True)
    with open(os.path.join(HERE, 'dna2orfs.json'), 'w') as fh:
        json.dump({'cases': cases}, fh, indent=0, sort_keys=True)
        fh.write('\n')


if __name__ == '__main__':
    main()
