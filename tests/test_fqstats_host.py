"""fqstats' restatement (fqstats_expect) and the tool's host line loop
(genome_tools.py:85-124 restated; CPU only) against the reference's own output
in tests/golden/fqstats.json, exception names included."""

import numpy as np
import pytest

import fqstats_expect as fe
from magot_amd import genome_tools

CASES = fe.load()['cases']
NAMES = sorted(CASES)


def _file(case, tmp_path):
    path = str(tmp_path / 'reads.fastq')
    with open(path, 'wb') as fh:
        fh.write(case['text'].encode('latin-1'))
    return path


def test_the_goldens_hold_every_case_the_tool_must_meet():
    texts = {name: CASES[name]['text'].encode('latin-1') for name in NAMES}
    assert {'example', 'crlf', 'empty_file', 'one_line', 'empty_sequences_only', 'one_base',
            'no_final_lf_sequence', 'no_final_lf_quality', 'lone_cr_in_sequence'} <= set(NAMES)
    for k in range(4):
        assert texts['lines_mod4_%d' % k].count(b'\n') % 4 == k
    assert texts['one_base'].count(b'\n') == 12 and CASES['one_base']['out'].startswith(
        '3 reads\ntotal basepairs=1\n')
    assert CASES['empty_sequences_only']['out'].endswith('n25=False\nn50=False\nn75=False\n')
    assert CASES['empty_file']['exc'] == CASES['one_line']['exc'] == 'ZeroDivisionError'
    assert b'\r\n' in texts['crlf'] and b'\r' in texts['lone_cr_in_sequence'].replace(b'\r\n', b'')
    assert not texts['no_final_lf_sequence'].endswith(b'\n')
    assert texts['no_final_lf_sequence'].count(b'\n') % 4 == 1
    assert texts['no_final_lf_quality'].count(b'\n') % 4 == 3


@pytest.mark.parametrize('name', NAMES)
def test_restatement_equals_the_reference(name):
    case = CASES[name]
    assert fe.expected(case['text'].encode('latin-1')) == (case['out'], case['exc'])


@pytest.mark.parametrize('name', NAMES)
def test_host_loop_equals_the_reference(name, tmp_path, capfdbinary):
    case = CASES[name]
    exc = None
    try:
        genome_tools.fqstats(_file(case, tmp_path), native='False')
    except Exception as e:  # noqa: BLE001
        exc = type(e).__name__
    assert (capfdbinary.readouterr().out.decode('latin-1'), exc) == (case['out'], case['exc'])
    assert genome_tools.fqstats.last_path == ('fqstats', 'host', "native != 'True'")


def test_host_loop_equals_the_restatement(tmp_path, capfdbinary):
    """300 seeded small files: every residue of the line count, CRLF, no final LF"""
    rng = np.random.default_rng(20261020)
    raised = 0
    path = str(tmp_path / 'reads.fastq')
    for n in range(300):
        data = fe.random_fastq(rng, eol=b'\r\n' if n % 5 == 4 else b'\n')
        with open(path, 'wb') as fh:
            fh.write(data)
        exc = None
        try:
            genome_tools.fqstats(path, native='False')
        except ZeroDivisionError:
            exc = 'ZeroDivisionError'
        assert (capfdbinary.readouterr().out.decode('latin-1'), exc) == fe.expected(data), n
        raised += exc is not None
    assert 0 < raised < 300  # both outcomes are met


def test_histogram_form_of_the_restatement():
    lengths = [0, 0, 3, 7, 7, 7, 150, 150, 4096]
    vals, counts = np.unique(lengths, return_counts=True)
    assert fe.figures_from_histogram(vals, counts) == fe.figures(lengths)


def test_tool_is_registered_and_documented(tmp_path, capfdbinary):
    assert genome_tools.TOOLS['fqstats'] is genome_tools.fqstats
    assert 'fqstats' in genome_tools.__doc__
    case = CASES['example']
    assert genome_tools.main(['fqstats', _file(case, tmp_path), 'native=False']) == 0
    assert capfdbinary.readouterr().out.decode('latin-1') == case['out']
    for native in ('True', 'False'):  # a path, never literal text
        with pytest.raises(OSError):
            genome_tools.fqstats(str(tmp_path / 'absent.fastq'), native=native)
    assert capfdbinary.readouterr().out == b''
