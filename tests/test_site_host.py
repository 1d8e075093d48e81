"""composition_by_site on the host (genome_tools.py:488-503): the expectation
of site_expect.py and the tool's host loop against every run recorded from the
reference in tests/golden/site.json (stdout, exception names, both orders);
the C++ renderer (magot_site_render) against the expectation on seeded counts;
the reasons the device path declines for, which need no device; the
command-line parsing."""

import numpy as np
import pytest

import site_expect as se
from magot_amd import engine, genome_tools

GOLD = se.load()
NAMES = sorted(GOLD)


def recorded(case, order):
    if order == 'py2':
        return case['out_py2'], case['exc_py2']
    return case['out'], case['exc']


def test_the_recorded_inputs_are_the_cases_of_site_expect():
    cases = se.cases()
    assert sorted(cases) == NAMES
    for name, (text, note) in cases.items():
        assert GOLD[name]['note'] == note
        if text is None:
            assert GOLD[name]['text'] is None and GOLD[name]['gen'] == name
        else:
            assert GOLD[name]['text'].encode('latin-1') == text
    notes = {se.note_of(note, order) for _, note in cases.values() for order in se.ORDERS}
    assert notes == {'native', 'IndexError', 'ZeroDivisionError', 'text before the first header',
                     'no records'}
    # the two orders differ somewhere, and nothing is printed with an exception
    assert sum(GOLD[n]['exc'] != GOLD[n]['exc_py2'] for n in NAMES) >= 2
    for n in NAMES:
        for order in se.ORDERS:
            out, exc = recorded(GOLD[n], order)
            assert (out == '') == (exc is not None)
            note = se.note_of(GOLD[n]['note'], order)
            if note in ('IndexError', 'ZeroDivisionError'):
                assert exc == note
            if note == 'native':
                assert exc is None


def test_the_recorded_floats_show_every_form():
    text = ''.join(GOLD[n]['out'] for n in NAMES)
    for form in ('0.333333333333', '0.666666666667', '0.142857142857', '0.857142857143',
                 '\t1.0', '\t0.0', '3.33333333333e-05', '0.999966666667'):
        assert form in text, form


@pytest.mark.parametrize('order', se.ORDERS)
@pytest.mark.parametrize('name', NAMES)
def test_expectation_equals_the_reference(name, order):
    assert se.expected(se.text_of(GOLD[name]), order) == recorded(GOLD[name], order)


def _tool(path, capfdbinary, **kw):
    exc = None
    try:
        genome_tools.composition_by_site(path, **kw)
    except Exception as e:  # noqa: BLE001
        exc = type(e).__name__
    return capfdbinary.readouterr().out.decode('latin-1'), exc


@pytest.mark.parametrize('order', se.ORDERS)
@pytest.mark.parametrize('name', NAMES)
def test_host_loop_equals_the_reference(name, order, tmp_path, capfdbinary):
    path = str(tmp_path / 'aln.fa')
    with open(path, 'wb') as fh:
        fh.write(se.text_of(GOLD[name]))
    assert _tool(path, capfdbinary, order=order, native='False') == recorded(GOLD[name], order)
    assert genome_tools.composition_by_site.last_path == \
        ('composition_by_site', 'host', "native != 'True'")


def test_a_string_that_names_no_file_is_the_text(capfdbinary):
    """ensure_file's reading (magot_smallfuncs.py:32-43), on the host loop
    whatever ``native`` says"""
    case = GOLD['plain']
    for native in ('True', 'False'):
        out, exc = _tool(case['text'], capfdbinary, order='insertion', native=native)
        assert (out, exc) == (case['out'], None)
        assert genome_tools.composition_by_site.last_path[1] == 'host'
    assert genome_tools.composition_by_site.last_path == \
        ('composition_by_site', 'host', "native != 'True'")
    _tool(case['text'], capfdbinary)
    assert genome_tools.composition_by_site.last_path[2] == 'not a regular file'


@pytest.mark.parametrize('name', ['empty_file', 'text_before_header'])
def test_declines_that_need_no_device(name, tmp_path, capfdbinary):
    """the two reasons read from the file's first byte"""
    path = str(tmp_path / 'aln.fa')
    with open(path, 'wb') as fh:
        fh.write(se.text_of(GOLD[name]))
    for order in se.ORDERS:
        assert _tool(path, capfdbinary, order=order) == recorded(GOLD[name], order)
        assert genome_tools.composition_by_site.last_path == \
            ('composition_by_site', 'host', GOLD[name]['note'])


def test_a_stream_that_writes_in_part_gets_the_whole_text(monkeypatch):
    """an unbuffered stdout takes at most 2 GiB at a call (one write(2)) and
    returns the count: an alignment of 2 * 10^8 sites prints 6 GB"""
    case = GOLD['sevenths']

    class Raw(object):
        def __init__(self):
            self.got, self.calls = b'', 0

        def write(self, data):
            self.calls += 1
            part = bytes(data[:7])
            self.got += part
            return len(part)

        def flush(self):
            pass

    class Stdout(object):
        buffer = Raw()

        def flush(self):
            pass

    monkeypatch.setattr(genome_tools.sys, 'stdout', Stdout())
    genome_tools.composition_by_site(case['text'], order='insertion', native='False')
    genome_tools._write_bytes(np.frombuffer(b'0123456789', np.uint8), b'', b'abc')
    assert Stdout.buffer.got.decode('latin-1') == case['out'] + '0123456789abc'
    assert Stdout.buffer.calls > len(case['out']) // 7


def test_the_tool_is_registered_and_checks_its_order(tmp_path, capfdbinary):
    assert genome_tools.TOOLS['composition_by_site'] is genome_tools.composition_by_site
    assert 'composition_by_site' in genome_tools.__doc__
    with pytest.raises(ValueError):
        genome_tools.composition_by_site(str(tmp_path / 'absent.fa'), order='sorted')
    assert genome_tools.parse_argv(['composition_by_site', 'aln.fa', 'order=insertion',
                                    'native=False']) == \
        ('composition_by_site', ['aln.fa'], {'order': 'insertion', 'native': 'False'})
    path = str(tmp_path / 'aln.fa')
    with open(path, 'wb') as fh:
        fh.write(se.text_of(GOLD['thirds']))
    assert genome_tools.main(['composition_by_site', path, 'order=insertion', 'native=False']) == 0
    assert capfdbinary.readouterr().out.decode('latin-1') == GOLD['thirds']['out']


# ---------------------------------------------------------------------------
# magot_site_render
# ---------------------------------------------------------------------------

def _seeded_counts():
    rng = np.random.default_rng(20261020)
    blocks = [rng.integers(0, 4, (300, 4)), rng.integers(0, 70, (3000, 4)),
              rng.integers(0, 40000, (8000, 4)), rng.integers(0, 2 ** 32, (2000, 4))]
    counts = np.concatenate(blocks).astype(np.uint32)
    counts = counts[counts.any(axis=1)]
    edge = []
    for total in (3, 7, 63, 64, 65, 30000, 99999, 10 ** 6, 10 ** 7, 10 ** 8, 10 ** 9,
                  4 * 10 ** 9, 2 ** 32 - 1):
        # count equal to total, and shares down to e-10
        edge += [[total, 0, 0, 0], [0, 0, 0, total], [1, total - 1, 0, 0], [0, 1, 0, total - 1],
                 [3, 0, total - 3, 0], [total // 3, total - total // 3, 0, 0]]
    return np.concatenate([counts, np.array(edge, np.uint64).astype(np.uint32)])


def test_renderer_equals_the_expectation_on_seeded_counts():
    counts = _seeded_counts()
    assert len(counts) > 3 * 4096  # rendered over several ranges
    want = se.render(counts)
    for form in ('e-05', 'e-06', 'e-07', 'e-08', 'e-09', 'e-10', '1.0\t0.0\t0.0\t0.0'):
        assert form in want, form
    for threads in (0, 1, 3):
        assert engine.render_composition(counts, threads=threads).tobytes().decode() == want
    assert engine.render_composition(counts[:5], threads=8).tobytes().decode() == \
        se.render(counts[:5])
    assert engine.render_composition(np.zeros((0, 4), np.uint32)).tobytes() == b'a\tt\tc\tg\n'


def test_renderer_reports_the_first_empty_site():
    counts = _seeded_counts()[:9000].copy()
    counts[[8000, 5000, 8999]] = 0
    with pytest.raises(ZeroDivisionError, match='site 5000'):
        engine.render_composition(counts)
    with pytest.raises(ValueError):
        engine.render_composition(np.zeros((4, 3), np.uint32))


def test_the_shape_constants_are_exposed():
    lane, tile = engine.SiteCounts.sites_per_lane(), engine.SiteCounts.sites_per_tile()
    w4, w8 = engine.SiteCounts.widening_periods()
    strip = engine.SiteCounts.rows_per_strip()
    assert lane == 8 and tile % (64 * lane) == 0
    # a nibble holds 15, a byte 255: the periods may not exceed what they hold
    assert 1 <= w4 <= 15 and w8 % w4 == 0 and w8 // w4 * 15 <= 255 and strip % w8 == 0
