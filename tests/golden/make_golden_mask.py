"""Record what the REFERENCE's own mask_from_gff prints: tests/golden/mask_from_gff.json.

Runs only where the reference is installed (see make_golden.py, whose
lib2to3 copy this imports); the reference function (genome_tools.py:394-428)
runs unchanged, and nothing of its program text is stored: only inputs,
outputs, hashes and exception names.

The copy runs under Python 3, which differs from the Python 2 target in two
places this function touches: files are opened with universal newlines (a
lone '\\r' would end a line) and ``upper()`` / ``lower()`` / ``split()`` act on
non-ASCII characters.  Every input here is therefore ASCII (and free of the
0x1c-0x1f separators Python 3's ``str.split`` adds) and ends its lines with
'\\n' or '\\r\\n', never a lone '\\r'; on such inputs both Pythons print the same
bytes, except for the order of the contigs, which is a dict's: ``sha_py2``
re-orders the per-contig blocks with the CPython 2.7 order model
(oracle.magot_oracle.py2_dict_order).

Per case: the FASTA and GFF inputs (``fasta`` / ``gff``, or ``fasta_file`` /
``gff_file`` for the shipped O.biroi subset) and a list of runs, each with
  mask_type, overwrite_softmask, feature_type   the arguments
  exc      exception name, or null
  sha      sha256 of the captured stdout (Python 3: insertion order)
  text     the stdout in full when short
  contigs  the contig names in insertion order when the run printed the
           genome (null after an exception or an invalid-argument return)
  blocks   sha256 of each contig's '>name\\nsequence\\n', in that order
  sha_py2  sha256 of the stdout with the blocks in Python 2 dict order
  decline  why the native path must leave this run to the line loop, or null
           when it must take it (set here from the case's definition: it is
           part of the contract the tests check, not a reference output)

Usage:  python tests/golden/make_golden_mask.py
"""

import json
import os
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import make_golden  # noqa: E402
from make_golden import mo, sha  # noqa: E402

OBIROI_FA = 'O.biroi_refseqGenomeSubset.fasta'
OBIROI_GFF = 'O.biroi_NCBIrefseq_gff3Subset.gff'
KEEP_TEXT = 2048
MODES = [('soft', 'True'), ('soft', 'False'), ('hard', 'True'), ('hard', 'False')]


def gff(*rows):
    """rows of (seqid, type, start, stop) -> nine-column GFF lines."""
    return ''.join('%s\tsrc\t%s\t%s\t%s\t.\t+\t.\tID=f%d\n' % (r[0], r[1], r[2], r[3], i)
                   for i, r in enumerate(rows))


MIXED = 'acgtnACGTNryswkmbdhvRYSWKMBDHV-*0129xX@['


def cases():
    """name -> (fasta, gff, decline per mask_type {'soft':, 'hard':} or one
    reason for both, extra runs [(mask_type, overwrite, feature_type)])."""
    c = {}
    two = '>ctgA first contig\n' + MIXED + '\n' + MIXED[::-1] + '\n>ctgB\nacgtacgtacGTACGTACGTnnnnNNNN\n'
    c['basic'] = (two, gff(('ctgA', 'CDS', 3, 12), ('ctgA', 'gene', 1, 70), ('ctgB', 'CDS', 1, 28),
                           ('ctgA', 'CDS', '+40', ' 45 '), ('ctgA', 'exon', 20, 30)), None,
                  [('soft', 'T', 'gene'), ('hard', 'f', 'exon'), ('soft', 'TRUE', 'mRNA')])
    c['overlap_nested_duplicate_abutting'] = (
        two, gff(('ctgA', 'CDS', 5, 40), ('ctgA', 'CDS', 10, 20), ('ctgA', 'CDS', 5, 40),
                 ('ctgA', 'CDS', 41, 50), ('ctgA', 'CDS', 50, 64), ('ctgB', 'CDS', 28, 28),
                 ('ctgB', 'CDS', 1, 1)), None, [])
    c['noops'] = (two, gff(('ctgA', 'CDS', 30, 10), ('ctgA', 'CDS', 500, 400), ('ctgB', 'CDS', 5, 0),
                           ('ctgB', 'CDS', 7, 9), ('ctgA', 'CDS', 1, 0)), None, [])
    c['start_zero_stop_minus_one_noop'] = (two, gff(('ctgA', 'CDS', 0, -1), ('ctgB', 'CDS', 2, 3)),
                                           None, [])
    c['stop_past_end_then_later_feature'] = (
        two, gff(('ctgA', 'CDS', 70, 90), ('ctgA', 'CDS', 5, 8), ('ctgA', 'CDS', 79, 85)),
        {'soft': None, 'hard': 'hard mask past the contig end: the list grows'}, [])
    c['start_past_end'] = (
        two, gff(('ctgB', 'CDS', 40, 45), ('ctgB', 'CDS', 3, 4), ('ctgB', 'CDS', 30, 31)),
        {'soft': None, 'hard': 'hard mask past the contig end: the list grows'}, [])
    c['start_zero'] = (two, gff(('ctgA', 'CDS', 0, 200), ('ctgA', 'CDS', 3, 4)),
                       'start < 1: a negative index', [])
    c['start_negative'] = (two, gff(('ctgB', 'CDS', -5, 27)), 'start < 1: a negative index', [])
    # lst[22:10] is empty: nothing to lower-case, but 16 'N's are inserted at 22
    c['start_negative_empty_slice'] = (
        two, gff(('ctgB', 'CDS', -5, 10), ('ctgB', 'CDS', 24, 25)),
        {'soft': None, 'hard': 'start < 1: a negative index'}, [])
    c['stop_negative'] = (two, gff(('ctgB', 'CDS', 1, -1), ('ctgB', 'CDS', 2, 3)),
                          'stop < 0: a negative index', [])
    c['unknown_seqid'] = (two, gff(('ctgA', 'CDS', 1, 5), ('nope', 'CDS', 1, 5)),
                          'unknown seqid: KeyError', [])
    c['unknown_seqid_noop_line'] = (two, gff(('nope', 'CDS', 9, 2)), 'unknown seqid: KeyError', [])
    c['bad_integer'] = (two, gff(('ctgA', 'CDS', 1, 5), ('ctgA', 'CDS', '12a', 20)),
                        'bad integer: ValueError', [])
    c['float_integer'] = (two, gff(('ctgA', 'CDS', 1, '5.0')), 'bad integer: ValueError', [])
    c['empty_integer'] = (two, gff(('ctgA', 'CDS', '', 5)), 'bad integer: ValueError', [])
    c['comment_line_with_six_tabs'] = (
        '>#c1 x\nacgtACGTacgtACGT\n>c2\nTTTTtttt\n',
        '##gff-version 3\n#c1\tsrc\tCDS\t2\t5\t.\t+\t.\tID=a\n# c2\tsrc\tgene\t1\t2\n' +
        gff(('c2', 'CDS', 3, 6)), None, [])
    c['few_tabs_ignored'] = (two, 'ctgA\tsrc\tCDS\t1\t5\t.\nctgA\tsrc\tCDS\t2\t6\t.\t+\n', None, [])
    c['crlf'] = (two.replace('\n', '\r\n'), gff(('ctgA', 'CDS', 3, 12), ('ctgB', 'CDS', 27, 28))
                 .replace('\n', '\r\n'), None, [])
    c['no_final_newline'] = ('>a\nacgt\nACGT', gff(('a', 'CDS', 2, 7))[:-1], None, [])
    c['blank_lines'] = ('>a\nacgt\n\nACGT\n\n>b\n\ngg\n', '\n' + gff(('a', 'CDS', 4, 5)) + '\n', None, [])
    c['long_interval'] = ('>long\n' + ('ACGTacgtNn' * 6)[:60] * 90 + '\n>short\nacgt\n',
                          gff(('long', 'CDS', 10, 4500), ('long', 'CDS', 4000, 5400),
                              ('short', 'CDS', 1, 4)), None, [])
    many = ''.join('>%s\n%s\n' % (nm, 'acGT' * (i + 1))
                   for i, nm in enumerate(['scaffold%d' % k for k in range(1, 24)] + ['x', 'Y', 'chrM']))
    c['many_contigs'] = (many, gff(('scaffold3', 'CDS', 2, 9), ('chrM', 'CDS', 1, 50),
                                   ('scaffold23', 'CDS', 90, 92), ('x', 'CDS', 1, 1)), None, [])
    # FASTA files the native reader sees differently from the reference's loop
    g = gff(('a', 'CDS', 2, 3))
    c['fasta_space_after_gt'] = ('> a desc\nacgt\n>b\nGGCC\n', gff(('b', 'CDS', 2, 3)),
                                 "whitespace directly after '>'", [])
    c['fasta_bare_gt'] = ('>\nacgt\n>a\nGGCC\n', g, 'the native reader returns None', [])
    c['fasta_empty_contig'] = ('>a\nacgt\n>e\n>b\nGG\n', g, 'an empty contig', [])
    c['fasta_repeated_name'] = ('>a x\nacgt\n>b\nGG\n>a y\nTTtt\n', g, 'a repeated name', [])
    c['fasta_sequence_before_header'] = ('acgt\n>a\nGGCC\n', g,
                                         'sequence before the first header: KeyError', [])
    c['fasta_blank_line_first'] = ('\n>a\nGGCC\n', g, 'sequence before the first header: KeyError',
                                   [])
    c['header_only'] = ('>a\n>b two\n', '', 'an empty contig',
                        [('soft', 'perhaps', 'CDS'), ('medium', 'True', 'CDS')])
    c['header_only_feature'] = ('>a\n>b two\n', gff(('b', 'CDS', 1, 3)), 'an empty contig',
                                [('soft', 'perhaps', 'CDS')])
    c['invalid_arguments'] = (two, gff(('ctgA', 'CDS', 3, 12)), None,
                              [('soft', 'yes', 'CDS'), ('hard', '', 'CDS'), ('medium', 'True', 'CDS'),
                               ('Soft', 'False', 'CDS'), ('medium', 'True', 'mRNA'),
                               ('medium', 'no', 'CDS')])
    return c


def run(tools, fa, gf, mask_type, overwrite, feature_type):
    _, exc, out = make_golden.call(lambda: tools.mask_from_gff(
        fa, gf, mask_type=mask_type, overwrite_softmask=overwrite, feature_type=feature_type))
    return out, exc


def entry(out, exc, mask_type, overwrite, feature_type, decline):
    e = {'mask_type': mask_type, 'overwrite_softmask': overwrite, 'feature_type': feature_type,
         'exc': exc, 'sha': sha(out), 'contigs': None, 'blocks': None, 'sha_py2': sha(out),
         'decline': decline}
    if len(out) <= KEEP_TEXT:
        e['text'] = out
    if exc is None and (out == '' or out.startswith('>')):
        lines = out.split('\n')
        assert lines[-1] == '' and len(lines) % 2 == 1, 'two lines per contig'
        names = [ln[1:] for ln in lines[0:-1:2]]
        blocks = {nm: '>' + nm + '\n' + seq + '\n' for nm, seq in zip(names, lines[1:-1:2])}
        assert len(blocks) == len(names) and ''.join(blocks[nm] for nm in names) == out
        e['contigs'] = names
        e['blocks'] = [sha(blocks[nm]) for nm in names]
        e['sha_py2'] = sha(''.join(blocks[nm] for nm in mo.py2_dict_order(names)))
    return e


def main():
    make_golden.reference_module()
    import genome_tools as tools
    out = {}
    with tempfile.TemporaryDirectory() as tmp:
        fa, gf = os.path.join(tmp, 'in.fa'), os.path.join(tmp, 'in.gff')
        for name, (fasta, gfftext, decline, extra) in cases().items():
            assert all(ord(ch) < 128 for ch in fasta + gfftext)
            assert '\r' not in (fasta + gfftext).replace('\r\n', '')
            for path, text in ((fa, fasta), (gf, gfftext)):
                with open(path, 'w', encoding='latin-1', newline='') as fh:
                    fh.write(text)
            runs = []
            for mt, ow in MODES:
                why = decline.get(mt) if isinstance(decline, dict) else decline
                runs.append(entry(*run(tools, fa, gf, mt, ow, 'CDS'), mt, ow, 'CDS', why))
            for mt, ow, ft in extra:
                valid = mt in ('soft', 'hard') and ow in ('True', 'T', 'true', 't', 'TRUE', 'False',
                                                          'F', 'false', 'f', 'FALSE')
                why = (decline.get(mt) if isinstance(decline, dict) else decline) if valid \
                    else 'an invalid argument'
                runs.append(entry(*run(tools, fa, gf, mt, ow, ft), mt, ow, ft, why))
            out[name] = {'fasta': fasta, 'gff': gfftext, 'runs': runs}
            print(name, [(r['mask_type'], r['overwrite_softmask'], r['exc']) for r in runs],
                  flush=True)
        runs = []
        for ft in ('CDS', 'gene'):
            for mt, ow in MODES:
                runs.append(entry(*run(tools, os.path.join(HERE, OBIROI_FA),
                                       os.path.join(HERE, OBIROI_GFF), mt, ow, ft), mt, ow, ft, None))
        out['obiroi'] = {'fasta_file': OBIROI_FA, 'gff_file': OBIROI_GFF, 'runs': runs}
        print('obiroi', [r['sha'][:8] for r in runs], flush=True)
    with open(os.path.join(HERE, 'mask_from_gff.json'), 'w') as fh:
        json.dump({'cases': out}, fh, indent=0, sort_keys=True)
        fh.write('\n')


if __name__ == '__main__':
    main()
