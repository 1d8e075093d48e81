"""exclude_from_fasta and fasta2tab on the host (genome_tools.py:377-391,
:349-350; magot_smallfuncs.py:21-29): the restated loops of fasta_expect.py and
both tools with native='False' against every run recorded from the reference in
tests/golden/fasta.json (stdout, exceptions, both dict orders); the restated
tables and verdicts against each case's note; genome.fasta2tab; the TOOLS
entries and the command line's argument parsing."""

import pytest

import fasta_expect as fe
from magot_amd import engine, genome, genome_tools

GOLD = fe.load()
NAMES = sorted(GOLD)
# what this module is about: without both tools none of its tests says anything
EXCLUDE, FASTA2TAB = genome_tools.TOOLS['exclude_from_fasta'], genome_tools.TOOLS['fasta2tab']


def b(text):
    return text.encode('latin-1')


def recorded(case, order):
    return case['out_py2'] if order == 'py2' else case['out']


def test_the_recorded_inputs_are_the_cases_of_fasta_expect():
    cases = fe.cases()
    assert sorted(cases) == NAMES
    for name, case in cases.items():
        g = GOLD[name]
        assert (b(g['fasta']), g['kind'], b(g['list']), g['first_word']) == \
            (case['fasta'], case['kind'], case['list'], case['first_word'])
        assert (g['path'], g['tab_path']) == fe.notes(case), name
    assert {GOLD[n]['path'] for n in NAMES} == \
        {'native', 'leading_text', 'stray_cr', 'a key without a word'}
    assert {GOLD[n]['exc'] for n in NAMES} == {None, 'IndexError'}
    assert {GOLD[n]['tab_exc'] for n in NAMES} == {None, 'IndexError'}
    assert sum(GOLD[n]['out_py2'] != GOLD[n]['out'] for n in NAMES) >= 3
    assert sum(GOLD[n]['path'] == 'native' for n in NAMES) * 4 >= len(NAMES) * 3


def test_the_reference_printed_what_the_issue_observed():
    want = {'issue_list_file': ('>a x\nGG\n>c y\nTT\n> \nAA\n', None),
            'issue_first_word': ('>a x\nGG\n', 'IndexError'),
            'issue_literal': ('>a x\nGG\n> \nAA\n', None)}
    for name, (out, exc) in want.items():
        assert (GOLD[name]['out'], GOLD[name]['exc']) == (out, exc)
        assert (GOLD[name]['tab_out'], GOLD[name]['tab_exc']) == \
            ('a x\tACGT\nb\t\nc y\tTT\na x\tGG\n \tAA\n', None)
    assert (GOLD['empty_file']['tab_out'], GOLD['empty_file']['out']) == ('\n', '')
    assert (GOLD['leading_text']['tab_out'], GOLD['leading_text']['tab_exc']) == ('', 'IndexError')


@pytest.mark.parametrize('order', fe.ORDERS)
@pytest.mark.parametrize('name', NAMES)
def test_restated_loops_equal_the_reference(name, order):
    case = GOLD[name]
    names = fe.exclusion_names(case['kind'], b(case['list']))
    out, exc = fe.expected_exclude(b(case['fasta']), names, case['first_word'], order)
    assert (out.decode('latin-1'), exc) == (recorded(case, order), case['exc'])
    out, exc = fe.expected_tab(b(case['fasta']))
    assert (out.decode('latin-1'), exc) == (case['tab_out'], case['tab_exc'])


@pytest.mark.parametrize('name', NAMES)
def test_tables_membership_and_pieces_give_the_recorded_text(name):
    """The restated tables of the device path lead to the reference's bytes:
    the GPU tests may compare the device against them."""
    case = GOLD[name]
    data = b(case['fasta'])
    t = fe.with_lines(fe.table(data), data)
    assert t['n_lines'] == len(fe.lines_of(data))
    assert fe.native_path(data) == ('native' if case['path'] == 'a key without a word'
                                    else case['path'])
    if t['verdict'] is not None:
        return
    assert [k[0] for k in t['keys']] == list(fe.sequence_dict(data))
    names = fe.exclusion_names(case['kind'], b(case['list']))

    def rendered(recs, style):
        out = bytearray(sum(n for _, _, n in fe.pieces(t, recs, style, 4)) + 3 * len(recs))
        at = 0
        for r in recs:  # the literal bytes, then the copies
            seq_len, name_len = t['records'][r][3], t['records'][r][2]
            if style == 'fasta':
                out[at] = ord('>')
                at += 1
            out[at + name_len] = ord('\n' if style == 'fasta' else '\t')
            at += name_len + 1 + seq_len + 1
            out[at - 1] = ord('\n')
        del out[at:]
        for src, dst, n in fe.pieces(t, recs, style, 4):
            out[dst:dst + n] = data[src:src + n]
        return bytes(out)

    if case['tab_exc'] is None:
        assert rendered(range(len(t['records'])), 'tab').decode('latin-1') == \
            (case['tab_out'] if t['records'] else '')
    if case['exc'] is None:
        keep = fe.member(t, names, case['first_word'])
        recs = [k[2] for k, kept in zip(t['keys'], keep) if kept]
        assert rendered(recs, 'fasta').decode('latin-1') == case['out']


def _call(fn, capfdbinary, *args, **kw):
    exc = None
    try:
        fn(*args, **kw)
    except Exception as e:  # noqa: BLE001
        exc = type(e).__name__
    return capfdbinary.readouterr().out.decode('latin-1'), exc


def write_case(tmp_path, case):
    """(the FASTA's path, the exclude_list argument) of a recorded case"""
    path = str(tmp_path / 'records.fa')
    with open(path, 'wb') as fh:
        fh.write(b(case['fasta']))
    if case['kind'] == 'literal':
        return path, case['list']
    list_path = str(tmp_path / 'names.txt')
    with open(list_path, 'wb') as fh:
        fh.write(b(case['list']))
    return path, list_path


@pytest.mark.parametrize('order', fe.ORDERS)
@pytest.mark.parametrize('name', NAMES)
def test_host_loop_equals_the_reference(name, order, tmp_path, capfdbinary):
    case = GOLD[name]
    path, arg = write_case(tmp_path, case)
    flag = 'True' if case['first_word'] else 'False'
    got = _call(genome_tools.exclude_from_fasta, capfdbinary, path, arg, flag, order=order,
                native='False')
    assert got == (recorded(case, order), case['exc'])
    assert genome_tools.exclude_from_fasta.last_path == \
        ('exclude_from_fasta', 'host', "native != 'True'")
    # a string that names no file is the text itself
    got = _call(genome_tools.exclude_from_fasta, capfdbinary, case['fasta'], arg, flag,
                order=order)
    assert got == (recorded(case, order), case['exc'])
    assert genome_tools.exclude_from_fasta.last_path == \
        ('exclude_from_fasta', 'host', 'not a regular file')


@pytest.mark.parametrize('name', NAMES)
def test_fasta2tab_on_the_host_equals_the_reference(name, tmp_path, capfdbinary):
    case = GOLD[name]
    path, _ = write_case(tmp_path, case)
    got = _call(genome_tools.fasta2tab, capfdbinary, path, native='False')
    assert got == (case['tab_out'], case['tab_exc'])
    assert genome_tools.fasta2tab.last_path == ('fasta2tab', 'host', "native != 'True'")
    if case['tab_exc'] is None:
        assert genome.fasta2tab(path) + '\n' == case['tab_out']
        if case['fasta']:
            assert genome.fasta2tab(case['fasta']) + '\n' == case['tab_out']
    else:
        with pytest.raises(IndexError):
            genome.fasta2tab(path)


def test_the_tools_are_registered_and_check_their_arguments(tmp_path, capfdbinary):
    assert genome_tools.TOOLS['exclude_from_fasta'] is genome_tools.exclude_from_fasta
    assert genome_tools.TOOLS['fasta2tab'] is genome_tools.fasta2tab
    with pytest.raises(ValueError):
        genome_tools.exclude_from_fasta(str(tmp_path / 'absent.fa'), 'a', order='sorted')
    assert capfdbinary.readouterr().out == b''
    assert engine.FastaRecords.PASSES[-1] == 'copy'
    assert engine._lib.FASTAREC_REASONS[1:] == ('leading_text', 'stray_cr', 'long_name',
                                                'hash_collision', 'too_large', 'too_many_lines')


def test_parse_argv_round_trips():
    assert genome_tools.parse_argv(['exclude_from_fasta', 'g.fa', 'a,b', 'just_firstword=True',
                                    'order=insertion']) == \
        ('exclude_from_fasta', ['g.fa', 'a,b'], {'just_firstword': 'True', 'order': 'insertion'})
    assert genome_tools.parse_argv(['fasta2tab', 'g.fa', 'native=False']) == \
        ('fasta2tab', ['g.fa'], {'native': 'False'})


def test_main_runs_both_tools_on_the_host(tmp_path, capfdbinary):
    case = GOLD['issue_literal']
    path, arg = write_case(tmp_path, case)
    assert genome_tools.main(['exclude_from_fasta', path, arg, 'native=False']) == 0
    assert capfdbinary.readouterr().out.decode('latin-1') == case['out_py2']
    assert genome_tools.main(['fasta2tab', path, 'native=False']) == 0
    assert capfdbinary.readouterr().out.decode('latin-1') == case['tab_out']


def test_the_worlds_tables_are_consistent_with_the_loops():
    for n, shape in ((1, 'mix'), (65, 'one'), (257, 'mix'), (257, 'distinct')):
        data = fe.world(n, shape)
        t = fe.table(data)
        assert t['verdict'] is None and len(t['records']) == n
        assert [k[0] for k in t['keys']] == list(fe.sequence_dict(data))
        assert [data[r[1]:r[1] + r[2]] for r in t['records']] == [r[4] for r in t['records']]
        assert [data[r[5]:r[5] + r[6]] for r in t['records']] == [r[7] for r in t['records']]
