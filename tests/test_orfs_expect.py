"""dna2orfs without a device: the closed-form expectation (tests/orfs_expect.py)
pinned to what the reference itself wrote (tests/golden/dna2orfs.json), the
tool's registration and its reference truthiness."""

import json
import os

import pytest

import orfs_expect as oe
from magot_amd import engine, genome_tools
from oracle import magot_oracle as mo


@pytest.fixture(scope='module')
def golden(golden_dir):
    with open(os.path.join(golden_dir, 'dna2orfs.json')) as fh:
        return json.load(fh)['cases']


def case_contigs(name, case, golden_dir):
    if 'input_file' in case:
        path = os.path.join(golden_dir, case['input_file'])
        with open(path, encoding='latin-1', newline='') as fh:
            assert oe.sha(fh.read()) == case['input_sha']
        return list(mo.read_fasta(path).items())
    contigs = oe.CASES[name]()
    text = oe.fasta(contigs)
    assert oe.sha(text) == case['input_sha']
    if 'input' in case:
        assert text == case['input']
    return contigs


def test_tile_constant():
    assert oe.TILE == engine.ORFCALL_TILE


def test_every_case_is_recorded(golden):
    assert set(golden) == set(oe.CASES) | {'obiroi'}


@pytest.mark.parametrize('name', sorted(oe.CASES) + ['obiroi'])
def test_helper_matches_reference(name, golden, golden_dir):
    case = golden[name]
    contigs = case_contigs(name, case, golden_dir)
    for from_atg, longest in oe.MODES:
        want = case['modes']['%d%d' % (from_atg, longest)]
        text, exc = oe.tool_text(contigs, from_atg, longest)
        assert exc == want['exc']
        assert oe.sha(text) == want['sha']
        if 'text' in want:
            assert text == want['text']
        blocks = [oe.sha(oe.block(nm, seq, from_atg, longest)[0]) for nm, seq in contigs]
        assert blocks == want['blocks']
        text, exc = oe.tool_text(contigs, from_atg, longest, order='py2')
        assert (oe.sha(text), exc) == (want['sha_py2'], want['exc_py2'])


def test_short_contigs_fail_as_the_reference_does(golden):
    for n in (1, 2, 3, 4):
        for mode in golden['short%d' % n]['modes'].values():
            assert mode['exc'] == 'AttributeError'


def test_tie_cases_are_ties():
    m, w = oe.longest_ties(oe.TIE_ACROSS, False)
    assert m == 29 and 1 in w and 2 in w and 0 not in w   # 0+ and 1-, not 0-
    m, w = oe.longest_ties(oe.TIE_ACROSS_ATG, True)
    assert m > 1 and 1 in w and 2 in w and 0 not in w
    for seq, from_atg in ((oe.TIE_INSIDE, False), (oe.TIE_INSIDE_ATG, True)):
        m, w = oe.longest_ties(seq, from_atg)
        assert m > 1 and len(w) >= 2 and w[0] == w[1]


def test_dna2orfs_is_a_tool():
    assert genome_tools.TOOLS['dna2orfs'] is genome_tools.dna2orfs
    assert 'dna2orfs' in genome_tools.__doc__


def test_command_line_truthiness(tmp_path, monkeypatch):
    """Command-line values are strings and the reference tests them as they
    are: ``from_atg=False`` switches from_atg on."""
    seen = []

    def fake(fasta, from_atg, longest, order):
        seen.append((from_atg, longest, order))
        return b'text'

    monkeypatch.setattr(genome_tools, '_dna2orfs_native', fake)
    fa = tmp_path / 'g.fa'
    fa.write_text('>a\nACGTACGT\n')
    out = tmp_path / 'o.fa'
    for argv, want in (
            (['from_atg=False'], (True, False, 'py2')),
            (['longest=0', 'order=insertion'], (False, True, 'insertion')),
            ([], (False, False, 'py2')),
            (['from_atg=1', 'longest=1'], (True, True, 'py2'))):
        name, args, kw = genome_tools.parse_argv(['dna2orfs', str(fa), str(out)] + argv)
        assert name == 'dna2orfs' and all(isinstance(v, str) for v in kw.values())
        genome_tools.TOOLS[name](*args, **kw)
        assert seen[-1] == want
        assert out.read_bytes() == b'text'
