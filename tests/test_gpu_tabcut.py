"""tab2fasta and repeatmasker2augustushints on the device (engine.TabCut,
tabcut.hip): every case of tests/golden/tabcut.json through native='True'
against the host path's bytes and the reference's recorded ones, the path each
call took, the kernels' own edges (text blocks, the 256-byte slices of the
n + 1 tables, the piece size, the copy's groups, a line that borrows no TAB of
its neighbour), magot_tabcut_rows against the restated line model on a seeded
table, the declines and the programs the ABI refuses."""

import numpy as np
import pytest

import goldlib
import tabcut_expect as te
from magot_amd import _lib, engine, genome_tools

pytestmark = pytest.mark.gpu

CASES = te.load()['cases']
NAMES = sorted(CASES)


def b(text):
    return text.encode('latin-1')


def _call(fn, capfdbinary, *args, **kw):
    exc = None
    try:
        fn(*args, **kw)
    except Exception as e:  # noqa: BLE001
        exc = type(e).__name__
    return capfdbinary.readouterr().out, exc


def written(tmp_path, data, name='table.tab'):
    path = str(tmp_path / name)
    with open(path, 'wb') as fh:
        fh.write(data)
    return path


def both_paths(fn, capfdbinary, path):
    """((stdout, exception) on the device, the same on the host, the device call's path)"""
    native = _call(fn, capfdbinary, path)
    took = fn.last_path
    host = _call(fn, capfdbinary, path, native='False')
    return native, host, took


def test_params_are_what_the_host_tests_assume():
    assert engine.TabCut.params() == te.PARAMS


def test_align_pep_tab_has_the_reference_checksum_on_the_device(capfdbinary):
    out, exc = _call(genome_tools.tab2fasta, capfdbinary, te.ALIGN)
    assert exc is None and goldlib.posix_cksum(out) == te.ALIGN_CKSUM
    assert genome_tools.tab2fasta.last_path == ('tab2fasta', 'native', None)


@pytest.mark.parametrize('name', NAMES)
def test_tab2fasta_on_the_device_equals_host_and_reference(name, tmp_path, capfdbinary):
    case = CASES[name]
    path = written(tmp_path, b(case['text']))
    native, host, took = both_paths(genome_tools.tab2fasta, capfdbinary, path)
    assert native == host
    assert native == (b(case['fasta_out']), case['fasta_exc'])  # an IndexError prints nothing
    if case['fasta_path'] == 'native':
        assert took == ('tab2fasta', 'native', None)
    else:
        assert took == ('tab2fasta', 'host', case['fasta_path'])


@pytest.mark.parametrize('name', NAMES)
def test_hints_on_the_device_equal_host_and_reference(name, tmp_path, capfdbinary):
    case = CASES[name]
    path = written(tmp_path, b(case['text']))
    native, host, took = both_paths(genome_tools.repeatmasker2augustushints, capfdbinary, path)
    assert native == host == (b(case['hints_out']), case['hints_exc'])
    assert took == ('repeatmasker2augustushints', 'native', None)  # a CR declines nothing here


def test_a_line_of_one_mebibyte(tmp_path, capfdbinary):
    """One field of 2^20 bytes is 256 pieces of as many lanes, in both tools."""
    big = te._seq(1 << 20)
    data = b'first\tshort\n' + b'name\t' + big + b'\tc\td\te\tf\tg\th\n' + b'last\tx\n'
    path = written(tmp_path, data)
    native, host, took = both_paths(genome_tools.tab2fasta, capfdbinary, path)
    assert native == host == (b'>first\nshort\n>name\n' + big + b'\n>last\nx\n', None)
    assert took[1] == 'native'
    native, host, took = both_paths(genome_tools.repeatmasker2augustushints, capfdbinary, path)
    assert native == host and native[0].startswith(b'name\t' + big + b'\tnonexonpart\td\te\tf\t.')
    assert took[1] == 'native'
    cut = engine.TabCut.parse(data, **te.TAB2FASTA)
    try:
        assert cut.n_pieces == 5 * 3 + 255  # 256 pieces for the field
    finally:
        cut.close()


@pytest.mark.parametrize('program', ('TAB2FASTA', 'HINTS'))
def test_rows_equal_the_line_model_on_a_seeded_table(program):
    """2,000 lines of 0 to 9 TABs and fields of 0 to 40 bytes: every line's
    verdict and output offset, the sizes and the rendered bytes."""
    data = te.random_table()
    prog = getattr(te, program)
    assert getattr(engine.TabCut, program) == prog
    want = te.rows_model(data, **prog)
    assert len(want['verdict']) == 2000 and len(set(want['verdict'])) == 2
    cut = engine.TabCut.parse(data, **prog)
    try:
        rows = cut.rows()
        assert rows['verdict'].tolist() == want['verdict']
        assert rows['offset'].tolist() == want['offset']
        assert (cut.n_lines, cut.n_tabs, cut.n_kept, cut.n_pieces, cut.out_bytes) == \
            (2000, want['n_tabs'], want['n_kept'], want['n_pieces'], len(want['out']))
        assert cut.short_line == want['short_line']
        assert cut.render().tobytes() == want['out']
        ms = cut.time(1)  # every pass again on the handle's own buffers: the answers stand
        assert set(ms) == set(engine.TabCut.PASSES) | {'text_bytes', 'out_bytes'}
        assert (ms['text_bytes'], ms['out_bytes']) == (len(data), len(want['out']))
        assert cut.rows()['offset'].tolist() == want['offset']
        assert cut.render().tobytes() == want['out']
    finally:
        cut.close()


@pytest.mark.parametrize('name,line', (('short_first', 0), ('short_last', 2), ('short_twice', 1),
                                       ('empty_line', 0), ('empty_last_line', 1)))
def test_sizes_report_the_lowest_short_line(name, line):
    cut = engine.TabCut.parse(b(CASES[name]['text']), **te.TAB2FASTA)
    try:
        assert cut.short_line == line
        assert cut.rows()['verdict'][line] == _lib.TABCUT_SHORT_LINE
    finally:
        cut.close()


def test_a_short_line_does_not_borrow_the_next_lines_tabs():
    """5, 6 and 7 TABs side by side in every order: only the 5 is skipped."""
    for name in NAMES:
        if not name.startswith('tabs_') or name == 'tabs_5000':
            continue
        cut = engine.TabCut.parse(b(CASES[name]['text']), **te.HINTS)
        try:
            want = [_lib.TABCUT_KEPT if n != '5' else _lib.TABCUT_SKIPPED for n in name[5:]]
            assert cut.rows()['verdict'].tolist() == want, name
            assert cut.short_line is None
        finally:
            cut.close()


def test_the_declines(tmp_path, capfdbinary):
    data = b(CASES['stray_cr_mid_line']['text'])
    assert engine.TabCut.parse(data, **te.TAB2FASTA) == (None, 'stray_cr')
    cut = engine.TabCut.parse(data, **te.HINTS)  # no CR check in the hints' program
    assert not isinstance(cut, tuple)
    cut.close()
    assert engine.TabCut.parse(b'a\tb\n' * 100, max_bytes=399, **te.TAB2FASTA) == \
        (None, 'too_large')
    # the host path then prints the reference's bytes
    path = written(tmp_path, data)
    out, exc = _call(genome_tools.tab2fasta, capfdbinary, path)
    assert (out, exc) == (b(CASES['stray_cr_mid_line']['fasta_out']), None)
    assert genome_tools.tab2fasta.last_path == ('tab2fasta', 'host', 'stray_cr')


def test_a_bad_program_is_an_argument_error():
    def refused(**kw):
        prog = dict(te.TAB2FASTA)
        prog.update(kw)
        with pytest.raises(_lib.MagotError) as err:
            engine.TabCut.parse(b'a\tb\n', **prog)
        assert 'status %d' % _lib.ERR_ARG in str(err.value)

    refused(items=(b'x',) * 9)            # more than max_items
    refused(items=((0, 2),))              # a field above need
    refused(items=((1, 0),))              # a range that decreases
    rows, blob = engine.TabCut.lower((b'abc',))
    for a, n in ((0, 4), (4, 0), (2, 2), (0xffffffff, 2)):  # a literal outside the blob
        rows['a'], rows['b'] = a, n
        cut = engine.TabCut()
        cut.ctx = _lib.default_context()
        with pytest.raises(_lib.MagotError) as err:
            cut._open(np.frombuffer(b'a\tb\n', np.uint8), rows, blob, 1, 1, True, 0)
        assert 'status %d' % _lib.ERR_ARG in str(err.value)
    rows['kind'], rows['a'], rows['b'] = 7, 0, 1  # no known kind
    cut = engine.TabCut()
    cut.ctx = _lib.default_context()
    with pytest.raises(_lib.MagotError):
        cut._open(np.frombuffer(b'a\tb\n', np.uint8), rows, blob, 1, 1, True, 0)
    with pytest.raises(_lib.MagotError):  # neither skip nor error
        cut._open(np.frombuffer(b'a\tb\n', np.uint8), *engine.TabCut.lower((b'abc',)), 1, 2,
                  True, 0)
