"""tab2fasta and repeatmasker2augustushints on the host (genome_tools.py:345-346
over magot_smallfuncs.py:12-18; genome_tools.py:449-454): the reference's own
checksum of Align.pep.tab, both tools with native='False' and genome.tab2fasta
against every run recorded from the reference in tests/golden/tabcut.json, the
restated loops and the cut program's line model against the same records, the
TOOLS entries and the command line."""

import os

import pytest

import goldlib
import tabcut_expect as te
from magot_amd import engine, genome, genome_tools

GOLD = te.load()
CASES = GOLD['cases']
NAMES = sorted(CASES)
# what this module is about: without both tools none of its tests says anything
TAB2FASTA = genome_tools.TOOLS['tab2fasta']
HINTS = genome_tools.TOOLS['repeatmasker2augustushints']


def b(text):
    return text.encode('latin-1')


def _call(fn, capfdbinary, *args, **kw):
    exc = None
    try:
        fn(*args, **kw)
    except Exception as e:  # noqa: BLE001
        exc = type(e).__name__
    return capfdbinary.readouterr().out.decode('latin-1'), exc


def write_case(tmp_path, case):
    path = str(tmp_path / 'table.tab')
    with open(path, 'wb') as fh:
        fh.write(b(case['text']))
    return path


def test_align_pep_tab_has_the_reference_checksum(capfdbinary):
    assert os.path.getsize(te.ALIGN) == 14869
    TAB2FASTA(te.ALIGN, native='False')
    out = capfdbinary.readouterr().out
    assert goldlib.posix_cksum(out) == te.ALIGN_CKSUM
    assert TAB2FASTA.last_path == ('tab2fasta', 'host', "native != 'True'")


def test_the_recorded_inputs_are_the_cases_of_tabcut_expect():
    cases = te.cases()
    assert sorted(cases) == NAMES
    for name, text in cases.items():
        assert b(CASES[name]['text']) == text, name
        assert CASES[name]['fasta_path'] == te.tab2fasta_path(text), name
    assert {CASES[n]['fasta_exc'] for n in NAMES} == {None, 'IndexError'}
    assert {CASES[n]['hints_exc'] for n in NAMES} == {None}
    assert {CASES[n]['fasta_path'] for n in NAMES} == {'native', 'stray_cr'}
    assert GOLD['absent'] in ('IOError', 'OSError', 'FileNotFoundError')
    assert sum(bool(CASES[n]['hints_out']) for n in NAMES) >= 10


def test_the_reference_printed_what_the_issue_observed():
    fasta = {'empty_file': ('\n', None), 'no_lf': ('>a\nb\n', None), 'one_line': ('>a\nb\n', None),
             'crlf': ('>a\nb\n', None), 'cr_at_the_end': ('>a\nb\n', None),
             'third_field_empty_crlf': ('>a\nb\n', None), 'third_field': ('>a\nb\n', None),
             'cr_in_fields': ('>ax\nyz\n', None), 'only_a_tab': ('>\n\n', None),
             'two_lines_no_lf': ('>a\nb\n>c\nd\n', None), 'no_tab': ('', 'IndexError'),
             'empty_line': ('', 'IndexError'), 'empty_last_line': ('', 'IndexError')}
    for name, want in fasta.items():
        assert (CASES[name]['fasta_out'], CASES[name]['fasta_exc']) == want, name
    hints = {'six_fields': '',
             'comment_short_and_no_lf': '#c\t2\tnonexonpart\t4\t5\t6\t.\t.\tpri=2;src=RM\n'
                                        '1\t\tnonexonpart\t\t\t\t.\t.\tpri=2;src=RM\n',
             'cr_in_hint_fields': 'a\r\tb\tnonexonpart\t\t\t\r\t.\t.\tpri=2;src=RM\n',
             'comments_only': ''}
    for name, want in hints.items():
        assert (CASES[name]['hints_out'], CASES[name]['hints_exc']) == (want, None), name


def test_the_shape_cases_have_their_shapes():
    cases = te.cases()
    for n in (4095, 4096, 4097, 8192):
        assert len(cases['size_%d' % n]) == n and CASES['size_%d' % n]['fasta_exc'] is None
    assert len(cases['size_4096_no_lf']) == 4096 and not cases['size_4096_no_lf'].endswith(b'\n')
    assert len(cases['straddle']) == 2 * te.PARAMS['text_block']
    assert CASES['straddle']['fasta_exc'] is None
    for n in (31, 32, 33, 64, 256):
        assert len(te.lines_of(cases['lines_%d' % n])) == n
        assert len(te.lines_of(cases['lines_%d_no_lf' % n])) == n
        assert not cases['lines_%d_no_lf' % n].endswith(b'\n')
    for n in (15, 16, 17, 33):
        assert te.rows_model(cases['pieces_%d' % n], **te.TAB2FASTA)['n_pieces'] == n
    # every destination residue mod 16 of a field's first byte
    offsets = te.rows_model(cases['names_0_to_17'], **te.TAB2FASTA)['offset']
    starts = {(o + 1 + k % 18 + 1) % 16 for k, o in enumerate(offsets)}
    assert starts == set(range(16))
    assert cases['tabs_5000'].count(b'\t') == 5 + 5000 + 6
    assert cases['tab_is_the_last_byte'].endswith(b'\t')
    assert b'\t' not in te.lines_of(cases['last_line_without_tab'])[-1]
    assert [te.rows_model(cases[n], **te.TAB2FASTA)['short_line']
            for n in ('short_first', 'short_last', 'short_twice')] == [0, 2, 1]


@pytest.mark.parametrize('name', NAMES)
def test_restated_loops_and_line_model_equal_the_reference(name):
    """The restated loops print the reference's bytes, and so does the cut
    program's model of a line where the device path is taken: the GPU tests may
    compare the device against either."""
    case = CASES[name]
    data = b(case['text'])
    out, exc = te.expected_tab2fasta(data)
    assert (out.decode('latin-1'), exc) == (case['fasta_out'], case['fasta_exc'])
    out, exc = te.expected_hints(data)
    assert (out.decode('latin-1'), exc) == (case['hints_out'], case['hints_exc'])
    model = te.rows_model(data, **te.HINTS)
    assert model['out'].decode('latin-1') == case['hints_out'] and model['short_line'] is None
    if case['fasta_path'] == 'native':
        model = te.rows_model(data, **te.TAB2FASTA)
        if case['fasta_exc']:
            assert model['short_line'] is not None
        else:
            assert model['short_line'] is None
            assert (model['out'] or b'\n').decode('latin-1') == case['fasta_out']


@pytest.mark.parametrize('name', NAMES)
def test_tab2fasta_on_the_host_equals_the_reference(name, tmp_path, capfdbinary):
    case = CASES[name]
    path = write_case(tmp_path, case)
    got = _call(genome_tools.tab2fasta, capfdbinary, path, native='False')
    assert got == (case['fasta_out'], case['fasta_exc'])  # an IndexError prints nothing
    assert genome_tools.tab2fasta.last_path == ('tab2fasta', 'host', "native != 'True'")
    if case['fasta_exc'] is None:
        assert genome.tab2fasta(path) + '\n' == case['fasta_out']
    else:
        with pytest.raises(IndexError):
            genome.tab2fasta(path)
    if case['literal_out'] is not None:  # a string that names no file is the text itself
        got = _call(genome_tools.tab2fasta, capfdbinary, case['text'])
        assert got == (case['literal_out'], case['literal_exc'])
        assert genome_tools.tab2fasta.last_path == ('tab2fasta', 'host', 'not a regular file')
        if case['literal_exc'] is None:
            assert genome.tab2fasta(case['text']) + '\n' == case['literal_out']


@pytest.mark.parametrize('name', NAMES)
def test_hints_on_the_host_equal_the_reference(name, tmp_path, capfdbinary):
    case = CASES[name]
    path = write_case(tmp_path, case)
    got = _call(genome_tools.repeatmasker2augustushints, capfdbinary, path, native='False')
    assert got == (case['hints_out'], case['hints_exc'])
    assert genome_tools.repeatmasker2augustushints.last_path == \
        ('repeatmasker2augustushints', 'host', "native != 'True'")


@pytest.mark.parametrize('native', ('True', 'False'))
def test_hints_of_a_path_that_does_not_open_raise_oserror(native, tmp_path, capfdbinary):
    with pytest.raises(OSError):
        genome_tools.repeatmasker2augustushints(str(tmp_path / 'absent.gff'), native=native)
    with pytest.raises(OSError):  # no literal-string input here
        genome_tools.repeatmasker2augustushints('a\tb\tc\td\te\tf\tg\n', native=native)
    assert capfdbinary.readouterr().out == b''


def test_the_tools_are_registered_and_described():
    assert genome_tools.TOOLS['tab2fasta'] is genome_tools.tab2fasta
    assert genome_tools.TOOLS['repeatmasker2augustushints'] is \
        genome_tools.repeatmasker2augustushints
    for tool in ('tab2fasta', 'repeatmasker2augustushints'):
        assert 'genome_tools %s <' % tool in genome_tools.__doc__
    assert engine.TabCut.PASSES[-1] == 'copy'
    assert engine._lib.TABCUT_REASONS[1:] == ('stray_cr', 'too_large', 'too_many_lines')
    for mine, theirs in ((engine.TabCut.TAB2FASTA, te.TAB2FASTA), (engine.TabCut.HINTS, te.HINTS)):
        assert mine == theirs
        assert len(mine['items']) <= te.PARAMS['max_items']


def test_parse_argv_round_trips():
    assert genome_tools.parse_argv(['tab2fasta', 'a.tab', 'native=False']) == \
        ('tab2fasta', ['a.tab'], {'native': 'False'})
    assert genome_tools.parse_argv(['repeatmasker2augustushints', 'rm.gff']) == \
        ('repeatmasker2augustushints', ['rm.gff'], {})


def test_main_runs_both_tools_on_the_host(tmp_path, capfdbinary):
    case = CASES['cr_in_hint_fields']
    path = write_case(tmp_path, case)
    assert genome_tools.main(['tab2fasta', path, 'native=False']) == 0
    assert capfdbinary.readouterr().out.decode('latin-1') == case['fasta_out']
    assert genome_tools.main(['repeatmasker2augustushints', path, 'native=False']) == 0
    assert capfdbinary.readouterr().out.decode('latin-1') == case['hints_out']


def test_fasta2tab_then_tab2fasta_gives_one_line_per_record(tmp_path, capfdbinary):
    fasta = b'>one two\nACGT\nAC\n>empty\n>three\r\nGG\r\nTT\n'
    path = str(tmp_path / 'records.fa')
    with open(path, 'wb') as fh:
        fh.write(fasta)
    genome_tools.fasta2tab(path, native='False')
    tab = capfdbinary.readouterr().out
    assert tab == b'one two\tACGTAC\nempty\t\nthree\tGGTT\n'
    tab_path = str(tmp_path / 'records.tab')
    with open(tab_path, 'wb') as fh:
        fh.write(tab)
    genome_tools.tab2fasta(tab_path, native='False')
    assert capfdbinary.readouterr().out == b'>one two\nACGTAC\n>empty\n\n>three\nGGTT\n'
