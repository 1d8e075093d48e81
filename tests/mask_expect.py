"""Shared by tests/test_mask_host.py and tests/test_gpu_mask.py: the golden
cases of tests/golden/mask_from_gff.json (the reference's own mask_from_gff
output, genome_tools.py:394-428), and a numpy restatement of what a coverage
array does to a contig.  Not a test module."""

import hashlib
import json
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')
KEEP = ('False', 'F', 'false', 'f', 'FALSE')


def sha(data):
    if isinstance(data, str):
        data = data.encode('latin-1')
    return hashlib.sha256(bytes(data)).hexdigest()


def load_cases():
    with open(os.path.join(GOLDEN, 'mask_from_gff.json')) as fh:
        return json.load(fh)['cases']


def case_inputs(case):
    """(fasta bytes, gff bytes) of a golden case."""
    if 'fasta_file' in case:
        with open(os.path.join(GOLDEN, case['fasta_file']), 'rb') as fh:
            fa = fh.read()
        with open(os.path.join(GOLDEN, case['gff_file']), 'rb') as fh:
            return fa, fh.read()
    return case['fasta'].encode('latin-1'), case['gff'].encode('latin-1')


def case_files(case, tmpdir):
    """Paths of a case's FASTA and GFF (written into tmpdir unless shipped)."""
    if 'fasta_file' in case:
        return os.path.join(GOLDEN, case['fasta_file']), os.path.join(GOLDEN, case['gff_file'])
    fa, gf = case_inputs(case)
    pa, pg = os.path.join(str(tmpdir), 'in.fa'), os.path.join(str(tmpdir), 'in.gff')
    with open(pa, 'wb') as fh:
        fh.write(fa)
    with open(pg, 'wb') as fh:
        fh.write(gf)
    return pa, pg


def run_id(run):
    return '%s-%s-%s' % (run['mask_type'], run['overwrite_softmask'] or 'empty', run['feature_type'])


def all_runs(cases):
    return [(name, i) for name in sorted(cases) for i in range(len(cases[name]['runs']))]


def apply_mask(seq, cov, hard, keep_case):
    """The masked contig (uint8) for a contig's bytes and one bool per base:
    upper() of everything unless the case is kept, then lower() or 'N' on
    the covered bases; both case changes touch ASCII letters only."""
    x = np.array(np.frombuffer(bytes(seq), np.uint8))
    cov = np.asarray(cov, bool)
    if not keep_case:
        x[(x >= ord('a')) & (x <= ord('z'))] -= 32
    if hard:
        x[cov] = ord('N')
    else:
        x[cov & (x >= ord('A')) & (x <= ord('Z'))] += 32
    return x


def coverage(intervals, lengths):
    """One bool array per contig from interval rows {contig, start, len}."""
    cov = [np.zeros(int(n), bool) for n in lengths]
    for c, s, n in zip(intervals['contig'].tolist(), intervals['start'].tolist(),
                       intervals['len'].tolist()):
        assert n > 0 and s + n <= len(cov[c]), 'every piece lies inside its contig'
        cov[c][s:s + n] = True
    return cov


def text_of(names, seqs):
    return b''.join(b'>' + nm.encode('latin-1') + b'\n' + bytes(s) + b'\n'
                    for nm, s in zip(names, seqs))


def first_mismatch(a, b):
    a, b = np.frombuffer(bytes(a), np.uint8), np.frombuffer(bytes(b), np.uint8)
    n = min(len(a), len(b))
    d = np.flatnonzero(a[:n] != b[:n])
    return int(d[0]) if len(d) else (None if len(a) == len(b) else n)
