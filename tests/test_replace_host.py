"""replace_names on the host (genome_tools.py:431-446): the tool with
native='False' and the restated loop of replace_expect.py against every run
recorded from the reference in tests/golden/replace.json (stdout, exceptions,
both dict orders); the field model the device path rests on against the same
records wherever a case's note says native; the tool's decision against the
notes; and a seeded fuzz of the property itself: inside the conditions the loop
over the keys and the field model print the same bytes."""

import random

import pytest

import replace_expect as rx
from magot_amd import engine, genome_tools

GOLD = rx.load()
NAMES = sorted(GOLD)
# what this module is about: without the tool none of its tests says anything
REPLACE = genome_tools.TOOLS['replace_names']


def b(text):
    return text.encode('latin-1')


def recorded(case, order):
    return case['out_py2'] if order == 'py2' else case['out']


def case_bytes(case):
    return b(case['text']), b(case['table']), b(case['name_end'])


def test_the_recorded_inputs_are_the_cases_of_replace_expect():
    cases = rx.cases()
    assert sorted(cases) == NAMES
    for name, case in cases.items():
        assert case_bytes(GOLD[name]) == (case['text'], case['table'], case['name_end']), name
        assert GOLD[name]['path'] == rx.notes(case), name
    notes = {GOLD[n]['path'][o] for n in NAMES for o in rx.ORDERS}
    assert notes == {'native', 'name_end', 'empty_name', 'long_name', 'delimiter_in_name',
                     'delimiter_in_value', 'chain', 'IndexError'}
    assert {GOLD[n]['exc'] for n in NAMES} == {None, 'IndexError'}
    assert sum(GOLD[n]['out_py2'] != GOLD[n]['out'] for n in NAMES) >= 3
    assert {GOLD[n]['name_end'] for n in NAMES} >= {' ', ';', '\t', '', ', '}


def test_the_reference_printed_what_the_issue_describes():
    # a two-field row's value carries its LF into the line
    assert GOLD['issue_two_fields']['out'] == 'G1\n G2\n gene10 x\nG2\n \n'
    assert GOLD['three_fields']['out'] == 'G1 G2 gene10 x\nG2 \n'
    assert GOLD['crlf_table']['out'] == 'AA\r\n BB c \r\nBB AA\r\n \r\n'
    assert GOLD['repeated_name']['out'] == 'last B last \n'
    # the last byte of a final line without LF goes
    assert GOLD['no_final_lf_name_and_d']['out'] == 'x y\nz G1\n'
    assert GOLD['no_final_lf_plain']['out'] == 'G1;gen\n'
    assert (GOLD['one_byte_text']['out'], GOLD['empty_text']['out']) == ('\n', '')
    assert (GOLD['tabless_line']['out'], GOLD['tabless_line']['exc']) == ('', 'IndexError')
    # the winner among nested names is the dict's first
    assert GOLD['nested_semicolon']['out'] != GOLD['nested_semicolon']['out_py2']


@pytest.mark.parametrize('order', rx.ORDERS)
@pytest.mark.parametrize('name', NAMES)
def test_restated_loop_equals_the_reference(name, order):
    case = GOLD[name]
    out, exc = rx.expected_loop(*case_bytes(case), order)
    assert (out.decode('latin-1'), exc) == (recorded(case, order), case['exc'])


@pytest.mark.parametrize('order', rx.ORDERS)
@pytest.mark.parametrize('name', NAMES)
def test_field_model_equals_the_reference_where_the_note_says_native(name, order):
    case = GOLD[name]
    if case['path'][order] == 'native':
        assert rx.expected_fields(*case_bytes(case), order).decode('latin-1') == \
            recorded(case, order)


def _call(fn, capfdbinary, *args, **kw):
    exc = None
    try:
        fn(*args, **kw)
    except Exception as e:  # noqa: BLE001
        exc = type(e).__name__
    return capfdbinary.readouterr().out.decode('latin-1'), exc


def write_case(tmp_path, case):
    path, table = str(tmp_path / 'text.txt'), str(tmp_path / 'names.tsv')
    with open(path, 'wb') as fh:
        fh.write(b(case['text']))
    with open(table, 'wb') as fh:
        fh.write(b(case['table']))
    return path, table


@pytest.mark.parametrize('order', rx.ORDERS)
@pytest.mark.parametrize('name', NAMES)
def test_host_loop_equals_the_reference(name, order, tmp_path, capfdbinary):
    case = GOLD[name]
    path, table = write_case(tmp_path, case)
    got = _call(genome_tools.replace_names, capfdbinary, path, table, case['name_end'],
                order=order, native='False')
    assert got == (recorded(case, order), case['exc'])
    if case['exc'] is None:
        assert genome_tools.replace_names.last_path == \
            ('replace_names', 'host', "native != 'True'")


@pytest.mark.parametrize('order', rx.ORDERS)
@pytest.mark.parametrize('name', NAMES)
def test_the_decision_is_the_note(name, order):
    case = GOLD[name]
    _, table, name_end = case_bytes(case)
    if case['exc'] == 'IndexError':
        with pytest.raises(IndexError):
            genome_tools._replace_table(table)
        return
    why, plan = genome_tools._replace_decline(genome_tools._replace_table(table), name_end, order)
    assert (why or 'native') == case['path'][order]
    if why is None:
        names, values, rank = plan
        assert (names, values) == rx.keyed(rx.table_rows(table))
        assert list(rank) == rx.ranks_of(names, name_end, order)


def test_py2_string_hashes_are_cpython_2_7s():
    from magot_amd import py2order
    keys = [b'', b'a', b'gene1;', b'\xff\xfe', b'x' * 300] + [b'%d;' % i for i in range(50)]
    want = [py2order.str_hash(k.decode('latin-1')) for k in keys]
    assert engine.py2_string_hashes(keys).tolist() == want
    assert engine.py2_string_hashes([]).tolist() == []


def test_a_missing_file_is_the_references_ioerror(tmp_path, capfdbinary):
    path, table = write_case(tmp_path, GOLD['issue_two_fields'])
    for args in ((str(tmp_path / 'absent.txt'), table), (path, str(tmp_path / 'absent.tsv'))):
        with pytest.raises(IOError):
            genome_tools.replace_names(*args)
        with pytest.raises(IOError):
            genome_tools.replace_names(*args, native='False')
    with pytest.raises(ValueError):
        genome_tools.replace_names(path, table, order='sorted')
    assert capfdbinary.readouterr().out == b''


def test_the_tool_is_registered_and_parses_its_arguments(tmp_path, capfdbinary):
    assert REPLACE is genome_tools.replace_names
    assert genome_tools.parse_argv(['replace_names', 't.gff', 'n.tsv', 'name_end=;',
                                    'order=insertion']) == \
        ('replace_names', ['t.gff', 'n.tsv'], {'name_end': ';', 'order': 'insertion'})
    case = GOLD['gff_ids']
    path, table = write_case(tmp_path, case)
    assert genome_tools.main(['replace_names', path, table, 'name_end=;', 'native=False']) == 0
    assert capfdbinary.readouterr().out.decode('latin-1') == case['out_py2']
    assert engine.NameReplacer.PASSES[-1] == 'copy'
    assert engine._lib.RENAME_REASONS[1:] == ('too_large', 'hash_collision', 'table_too_large')
    assert engine.NameReplacer.params() == rx.PARAMS


def test_fuzz_the_loop_and_the_field_model_agree_inside_the_conditions():
    """The property the device path rests on: 4000 seeded small cases; wherever
    the decision says native, the loop over the keys (the tool's own, and the
    restated one) prints what the field model prints."""
    rnd = random.Random(20261020)
    native = 0
    for _ in range(4000):
        text, table, d = rx.fuzz_case(rnd)
        for order in rx.ORDERS:
            want, exc = rx.expected_loop(text, table, d, order)
            assert exc is None
            rows = genome_tools._replace_table(table)
            names, values = genome_tools._replace_dict(rows, d, order)
            got = b''.join(genome_tools._replace_host(text, [n + d for n in names],
                                                      [v + d for v in values]))
            assert got == want
            why, _ = genome_tools._replace_decline(rows, d, order)
            assert (why or 'native') == rx.note(table, d, order)
            if why is None:
                native += 1
                assert rx.expected_fields(text, table, d, order) == want, (text, table, d, order)
    assert native >= 2000
