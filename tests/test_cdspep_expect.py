"""The closed form of tests/cdspep_expect.py against the reference's own
choice (oracle.magot_oracle.get_orfs), and the properties the device tests
rely on in its cases (CPU)."""

import pytest

import cdspep_expect as ce
import orfs_expect as oe
from oracle import magot_oracle as mo

S = 64  # engine.LongestOrfs.params()['step'] (the device tests take it from there)


def _choice(seq):
    try:
        return mo.get_orfs(seq, longest=True)
    except IndexError:
        return None


def test_expected_row_is_the_references_choice():
    contig, recs = ce.case_lengths()
    seqs = [contig[st:st + ln] for st, ln, _ in recs]
    seqs += ce.case_n_records() + ce.case_step_stops(S) + ce.case_step_ties(S)
    seqs += [s for name in ('n_lower', 'ties', 'stream_edges') for _, s in oe.CASES[name]()]
    for seq in seqs:
        row = ce.expected_row(seq)  # asserts the string itself
        if row is None:
            assert _choice(seq) is None
            continue
        j, k, orf = row
        t = oe.six_frames(seq)[j]
        assert t[k:k + len(orf)] == orf and (k == 0 or t[k - 1] == '*')
        assert k + len(orf) == len(t) or t[k + len(orf)] == '*'


def test_records_without_a_candidate():
    for seq in ('', 'A', 'AC', 'NNN', 'NNNN', 'nnnn', 'N-N'):
        assert ce.expected_row(seq) is None
    # five Ns: frame 1 drops its junk codon, not the real one behind it
    assert ce.expected_row('NNNNN') == (2, 0, 'X') and _choice('NNNNN') == 'X'
    assert ce.expected_row('ACG') == (0, 0, 'R')  # 0- comes first: CGT
    assert ce.expected_row('NNNTAAGCC') is not None


def test_custom_library_row():
    lib = dict(mo.STANDARD_CODE)
    lib['GCC'] = '*'
    assert ce.expected_row('GCCGCCATGAAA', lib) == (0, 0, 'FHGG')
    lut = ce.lut64_of(mo.STANDARD_CODE)
    assert len(lut) == 64 and lut[0:1] == b'K' and lut[63:64] == b'F' and lut[3:4] == b'*'


@pytest.fixture(scope='module')
def golden(golden_dir):
    import json
    import os
    with open(os.path.join(golden_dir, 'get_cds_peptides.json')) as fh:
        return json.load(fh)['cases']


@pytest.mark.parametrize('name', sorted(ce.TOOL_CASES))
def test_tool_closed_form_against_the_reference(name, golden, golden_dir):
    """The reference's own run (Python 3: insertion order) per case."""
    want = golden[name]
    fasta, gff, kw = ce.tool_inputs(name, golden_dir)
    assert (oe.sha(fasta), oe.sha(gff), kw) == (want['fasta_sha'], want['gff_sha'], want['kw'])
    entries, exc, printed = ce.walk(fasta, gff, order='insertion', **kw)
    text, exc2 = ce.tool_text(fasta, gff, order='insertion', **kw)
    assert exc == exc2 == want['exc']
    assert (text is not None) == want['file'] == (entries is not None)
    text = text or ''
    assert (oe.sha(text), len(text)) == (want['sha'], want['size'])
    if 'out' in want:
        assert text == want['out']
    assert printed == want['stdout']


def test_tool_cases_reach_what_they_are_for(golden):
    assert golden['nnn_middle']['exc'] == 'IndexError' and golden['nnn_middle']['size'] > 0
    assert golden['nnn_middle']['out'] != golden['basic']['out'][:golden['nnn_middle']['size']] or \
        golden['nnn_middle']['size'] < golden['basic']['size']
    assert golden['obiroi']['exc'] == 'KeyError' and golden['obiroi']['size'] == 0
    assert golden['names_invalid']['stdout'].count(ce.INVALID_NAMES) == 6  # once per transcript
    assert '>cA1.1dup\n' in golden['basic']['out'] and '>cA1.1a\n' not in golden['basic']['out']
    assert golden['length_below']['out'] != golden['length_above']['out']
    assert golden['c14']['exc'] is None and golden['c14']['size'] > 100000
    # no annotations at all: raised inside read_gff, before the output file is opened
    assert (golden['no_annotations']['exc'], golden['no_annotations']['file']) == \
        ('AttributeError', False)
    # no CDS line: the CDS dict exists all the same, an empty file and no exception
    none = golden['no_cds_lines']
    assert (none['exc'], none['file'], none['size']) == (None, True, 0)
    fa, gff = ce.synthetic_genome(), ce.synthetic_gff()
    for bad, exc in ce.DIAGNOSTICS.items():
        kw = {'gene_length_filter': '10'} if bad == 'no_second_line' else {}
        assert ce.walk(fa, ce.synthetic_gff(bad=bad), order='insertion', **kw)[1] == exc
    assert ce.walk(fa, gff, order='insertion')[1] is None


def test_case_properties():
    contig, recs = ce.case_lengths()
    assert {st % 16 for st, _, _ in recs} == set(range(16))
    assert sorted({ln for _, ln, _ in recs}) == list(range(201))
    for s in ce.case_open_run(S):
        assert all(len(max(t.split('*'), key=len)) > 3 * S for t in oe.six_frames(s))
    for q, s in enumerate(ce.case_step_ties(S)):
        m, tied = ce.tied_runs(s)
        assert m == S - 3 and len(tied) == 2
        assert tied[0][0] == tied[1][0] == (1 if q % 2 == 0 else 0)
        assert tied[0][1] // S == 0 and tied[1][1] // S == 1
    hit = set()
    for s in ce.case_step_stops(S)[:12:2]:
        hit.add(oe.six_frames(s)[1].index('*'))
    assert hit == {S - 2, S - 1, S, S + 1, 2 * S - 1, 2 * S}
