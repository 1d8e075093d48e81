"""besthits_from_psl on the host (genome_tools.py:572-592): the restated loop
of psl_expect.py and the tool with native='False' against every run recorded
from the reference in tests/golden/psl.json (stdout, exceptions, both dict
orders); the native grammar's restated verdict against each case's note; and
the two host functions of the device path -- magot_psl_order against
py2order.dict_order, magot_psl_render against the Python slice rule."""

import random

import numpy as np
import pytest

import psl_expect as pe
from magot_amd import engine, genome_tools, py2order

GOLD = pe.load()
NAMES = sorted(GOLD)
ORDERS = ('insertion', 'py2')


def recorded(case, order):
    if order == 'py2' and case['out_py2'] is not None:
        return case['out_py2']
    return case['out']


def test_the_recorded_inputs_are_the_cases_of_psl_expect():
    cases = pe.cases()
    assert sorted(cases) == NAMES
    for name, (text, path) in cases.items():
        assert GOLD[name]['text'].encode('latin-1') == text
        assert GOLD[name]['path'] == path
        assert pe.native_path(text) == path, name
    paths = {path for _, path in cases.values()}
    assert paths == {'native', 'few_fields', 'integer_form', 'number_range'}
    # the reference never raises, and an error case has one record
    assert all(GOLD[n]['exc'] is None for n in NAMES)
    assert sum(GOLD[n]['out_py2'] is None for n in NAMES) >= 6
    assert sum(GOLD[n]['out_py2'] not in (None, GOLD[n]['out']) for n in NAMES) >= 3


@pytest.mark.parametrize('order', ORDERS)
@pytest.mark.parametrize('name', NAMES)
def test_restated_loop_equals_the_reference(name, order):
    case = GOLD[name]
    got = pe.expected(case['text'].encode('latin-1'), order)
    assert got.decode('latin-1') == recorded(case, order)


@pytest.mark.parametrize('name', NAMES)
def test_table_and_loop_agree_on_native_cases(name):
    case = GOLD[name]
    if case['path'] != 'native':
        return
    text = case['text'].encode('latin-1')
    t = pe.table(text)
    rows = t['pass'] + [(g[4], g[5]) for g in t['groups']]
    want = b''.join(text[o:o + n - 1] + b'\n' for o, n in rows)
    assert want.decode('latin-1') == case['out']
    assert t['n_lines'] == len(pe.lines_of(text))


def _tool(tmp_path, case, capfdbinary, **kw):
    path = str(tmp_path / 'hits.psl')
    with open(path, 'wb') as fh:
        fh.write(case['text'].encode('latin-1'))
    exc = None
    try:
        genome_tools.besthits_from_psl(path, **kw)
    except Exception as e:  # noqa: BLE001
        exc = type(e).__name__
    return capfdbinary.readouterr().out.decode('latin-1'), exc


@pytest.mark.parametrize('order', ORDERS)
@pytest.mark.parametrize('name', NAMES)
def test_line_loop_equals_the_reference(name, order, tmp_path, capfdbinary):
    case = GOLD[name]
    out, exc = _tool(tmp_path, case, capfdbinary, order=order, native='False')
    assert (out, exc) == (recorded(case, order), case['exc'])
    assert genome_tools.besthits_from_psl.last_path == \
        ('besthits_from_psl', 'host', "native != 'True'")


def test_what_came_before_an_error_line_stays_printed():
    case = GOLD['few_fields_after_header']
    assert case['out'].startswith(pe.HEADER.decode('latin-1') + 'psl\n')
    assert case['out'].endswith('\n\n') and 'more' not in case['out']
    assert 'q1' not in case['out'].split('psl\n')[0]  # no winner was printed


def test_the_tool_is_registered_and_checks_its_order(tmp_path, capfdbinary):
    assert genome_tools.TOOLS['besthits_from_psl'] is genome_tools.besthits_from_psl
    with pytest.raises(ValueError):
        genome_tools.besthits_from_psl(str(tmp_path / 'absent.psl'), order='sorted')
    with pytest.raises(OSError):
        genome_tools.besthits_from_psl(str(tmp_path / 'absent.psl'), native='False')
    assert capfdbinary.readouterr().out == b''


# ---------------------------------------------------------------------------
# magot_psl_order
# ---------------------------------------------------------------------------

def _keys(n, seed):
    rnd = random.Random(seed)
    keys = set()
    while len(keys) < n:
        keys.add('q%x_%d' % (rnd.getrandbits(40), rnd.randrange(9)))
    keys = sorted(keys)
    rnd.shuffle(keys)
    return keys


def _assert_order(keys):
    hashes = np.array([py2order.str_hash(k) for k in keys], np.uint64)
    perm = engine.py2_order_of_hashes(hashes)
    assert perm.dtype == np.uint64 and len(perm) == len(keys)
    assert [keys[int(i)] for i in perm] == py2order.dict_order(keys)


@pytest.mark.parametrize('n', [0, 1, 5, 6, 1000, 60000])
def test_native_dict_order_equals_py2order(n):
    """5 -> 6 keys is the first resize; 60,000 crosses the `used > 50000` rule"""
    _assert_order(_keys(n, 20261020 + n))


def test_native_dict_order_on_keys_that_share_low_hash_bits():
    pool = _keys(40000, 7)
    for bits, want in ((3, 40), (10, 300)):
        low = py2order.str_hash(pool[0]) & ((1 << bits) - 1)
        same = [k for k in pool if py2order.str_hash(k) & ((1 << bits) - 1) == low]
        assert len(same) >= want // 8
        _assert_order(list(dict.fromkeys(same[:want] + pool[:20])))  # distinct, as the ABI asks


# ---------------------------------------------------------------------------
# magot_psl_render
# ---------------------------------------------------------------------------

def test_renderer_equals_the_slice_rule():
    text = b'first line\n\nabc\r\nlast without lf'
    rows = [(0, 11), (11, 1), (12, 5), (17, 15), (0, 11)]
    off, length = zip(*rows)
    got = engine.render_lines(text, off, length).tobytes()
    assert got == b''.join(text[o:o + n][:-1] + b'\n' for o, n in rows)
    assert got.endswith(b'last without l\nfirst line\n')
    whole = engine.render_lines(text, off, length, whole=True).tobytes()
    assert whole == b''.join(text[o:o + n] + b'\n' for o, n in rows)
    assert engine.render_lines(text, [], []).tobytes() == b''
    assert engine.render_lines(b'', [], []).tobytes() == b''
    assert engine.render_lines(b'', [0], [0], whole=True).tobytes() == b'\n'


def test_renderer_refuses_rows_outside_the_text():
    text = b'abc\n'
    for off, length in (([5], [1]), ([2], [3]), ([0], [0]), ([1 << 63], [1 << 63])):
        with pytest.raises(engine.MagotError):
            engine.render_lines(text, off, length)
