"""fqstats' read lengths on the device (engine.ReadLengths, fastq.hip) against
the restatement (fqstats_expect) and numpy.bincount, and, through
genome_tools.fqstats, against the reference's own output in
tests/golden/fqstats.json.  One text of a few MB whose shapes are the smallest
that reach every path: sequence lines around the lane, the wave-span, the text
block and the LDS histogram sizes, LFs on a block's and a chunk's first and
last byte, a CRLF split by a chunk seam, a text block of LFs only, lines longer
than a chunk and lengths around the dense bound, parsed in chunks of 4 KB (a
thousand seams), 64 KB and the default.

Not reachable by a test of this size: a file offset past 2^32 (offsets and
line counts are 64-bit throughout; a chunk's own are below 2^30)."""

import os
import subprocess
import sys

import numpy as np
import pytest

import fqstats_expect as fe
from magot_amd import _lib, engine, genome_tools

pytestmark = pytest.mark.gpu

BLOCK = 4096  # text bytes per workgroup round, and the smallest chunk used here
SMALL, MIDDLE = 4096, 65536
SEQ_LENGTHS = [0, 1, 15, 16, 17, 1023, 1024, 1025, 4095, 4096, 4097, 10000]
CASES = fe.load()['cases']
NAMES = sorted(CASES)
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


class Text(object):
    """FASTQ bytes built line by line, with lines sized to put their LF at a
    chosen offset mod BLOCK"""

    def __init__(self, rng):
        self.parts, self.size, self.lines, self.rng = [], 0, 0, rng

    def line(self, body, eol=b'\n'):
        self.parts += [body, eol]
        self.size += len(body) + len(eol)
        self.lines += 1

    def seq(self, n):
        return np.frombuffer(b'ACGTN', np.uint8)[self.rng.integers(0, 5, n)].tobytes()

    def fill_to(self, residue, first=b'@', eol=b'\n'):
        """A line whose last byte (its LF) lies at ``residue`` mod BLOCK"""
        body = (residue - self.size - (len(eol) - 1)) % BLOCK
        body = body or BLOCK
        self.line(first + b'x' * (body - 1), eol)
        assert (self.size - 1) % BLOCK == residue

    def record(self, n, eol=b'\n', quality=None):
        self.line(b'@r%d' % self.lines, eol)
        self.line(self.seq(n), eol)
        self.line(b'+', eol)
        self.line(b'I' * (n if quality is None else quality), eol)


class World(object):
    def __init__(self):
        rng = np.random.default_rng(20261020)
        self.dense = int(_lib.lib().magot_fq_dense())
        t = Text(rng)
        for n in SEQ_LENGTHS:
            t.record(n)
        for n in (61, 1030):  # a CR before the LF counts: 62 and 1031
            t.record(n, eol=b'\r\n')
        # a lone CR inside a sequence line is a base like any other
        t.line(b'@cr')
        t.line(b'ACGT\rACGT')
        t.line(b'+')
        t.line(b'IIII\rIIII')
        # a header's LF on the last byte of a text block (and of a 4 KB chunk):
        # the sequence line starts the next block
        t.fill_to(BLOCK - 1)
        self.lf_last = t.size - 1
        t.line(t.seq(700))
        t.line(b'+')
        t.line(b'I' * 700)
        # a header's LF on the first byte of a block
        t.fill_to(0)
        self.lf_first = t.size - 1
        t.line(t.seq(33))
        t.line(b'+')
        # a quality line's LF on the last byte of a block: the next record's
        # line index comes from the carry alone at 4 KB chunks
        t.fill_to(BLOCK - 1, first=b'I')
        # a header's CRLF split by a chunk seam, then a sequence line's
        t.fill_to(0, eol=b'\r\n')
        self.crlf_split = t.size - 2
        t.line(t.seq(50))
        t.line(b'+')
        t.line(b'I' * 50)
        t.line(b'@split')
        t.fill_to(0, first=b'A', eol=b'\r\n')
        self.crlf_split_seq = t.size - 2
        t.line(b'+')
        # two text blocks of LFs only: every fourth empty line is a read of 0
        t.fill_to(BLOCK - 1, first=b'I')
        self.lf_run = t.size
        for _ in range(2 * BLOCK):
            t.line(b'')
        # a wave's 1 KB span in which every sequence line has another length
        assert t.lines % 4 == 0
        self.distinct_at = t.size
        for n in range(1, 41):
            t.line(b'@')
            t.line(t.seq(n))
            t.line(b'+')
            t.line(b'I')
        # short reads: one length 3000 times
        for _ in range(3000):
            t.record(150)
        # around the dense bound: lines far longer than a chunk (no line is
        # looked into, so their quality lines can be short)
        for n in (self.dense - 1, self.dense, self.dense + 1):
            t.record(n, quality=7)
        # the last line lacks its LF and is a sequence line
        t.line(b'@last')
        t.line(b'ACGTACGTAC', eol=b'')
        self.text = b''.join(t.parts)
        assert len(self.text) == t.size
        self.lengths = fe.read_lengths(self.text)
        self.figures = fe.figures(self.lengths)
        self.parsed = {}

    def parse(self, chunk):
        if chunk not in self.parsed:
            self.parsed[chunk] = engine.ReadLengths.parse(self.text, chunk_bytes=chunk)
        return self.parsed[chunk]


@pytest.fixture(scope='module')
def world():
    w = World()
    text = w.text
    assert w.dense >= 1 << 20 and len(text) < 6 * w.dense
    # the shapes the docstring names are there
    assert text[w.lf_last] == 10 and w.lf_last % BLOCK == BLOCK - 1
    assert text[w.lf_first] == 10 and w.lf_first % BLOCK == 0
    for at in (w.crlf_split, w.crlf_split_seq):
        assert text[at:at + 2] == b'\r\n' and at % BLOCK == BLOCK - 1
    assert w.lf_run % BLOCK == 0 and text[w.lf_run:w.lf_run + 2 * BLOCK] == b'\n' * (2 * BLOCK)
    span = text[w.distinct_at:w.distinct_at + 1024]
    span = fe.read_lengths(span[:span.rindex(b'\n') + 1])
    assert w.distinct_at % 1024 == 0 and len(span) > 12 and len(set(span)) == len(span)
    assert not text.endswith(b'\n') and text.count(b'\n') % 4 == 1
    have = set(w.lengths)
    assert have >= set(SEQ_LENGTHS) | {w.dense - 1, w.dense, w.dense + 1, 9, 700, 33, 50}
    assert {62, 1031} <= have and not {61, 1030} & have  # a CR before the LF counts
    assert w.lengths.count(150) == 3000 and w.lengths.count(0) > 2 * BLOCK // 4
    assert w.lengths[-1] == 9  # ten bytes, recorded one short
    yield w
    for r in w.parsed.values():
        r.close()


@pytest.mark.parametrize('chunk', [SMALL, MIDDLE, 0])
def test_parse_equals_the_restatement(world, chunk):
    r = world.parse(chunk)
    f = world.figures
    assert (r.reads, r.bases) == (f['reads'], f['bases'])
    assert r.stats() == {k: f[k] for k in fe.KEYS}
    lengths, counts = r.histogram()
    binned = np.bincount(np.asarray(world.lengths, dtype=np.int64))
    occurs = np.flatnonzero(binned)
    assert lengths.dtype == np.int64 and counts.dtype == np.int64
    assert lengths.tolist() == occurs.tolist() and counts.tolist() == binned[occurs].tolist()
    assert lengths[-3:].tolist() == [world.dense - 1, world.dense, world.dense + 1]
    assert fe.figures_from_histogram(lengths, counts) == f


def test_chunk_sizes_agree_and_timing_changes_nothing(world):
    small, middle, whole = (world.parse(c) for c in (SMALL, MIDDLE, 0))
    assert small.stats() == middle.stats() == whole.stats()
    for a, b in zip(small.histogram() + middle.histogram(), whole.histogram() * 2):
        assert (a == b).all()
    before = whole.stats()
    ms = whole.time(1)
    assert set(ms) == {'line_index', 'lengths', 'reduce', 'copy', 'chunk_bytes'}
    assert ms['chunk_bytes'] == len(world.text) and ms['lengths'] > 0 and ms['reduce'] > 0
    assert small.time(1)['chunk_bytes'] == (len(world.text) - 1) % SMALL + 1
    assert whole.stats() == before
    # small's last chunk went through slot 0; one that went through slot 1
    last = len(world.text) - 1
    assert last // SMALL % 2 == 0 and last // (2 * MIDDLE) % 2 == 1
    even = engine.ReadLengths.parse(world.text, chunk_bytes=2 * MIDDLE)
    assert even.time(1)['chunk_bytes'] == (len(world.text) - 1) % (2 * MIDDLE) + 1
    assert even.stats() == before
    even.close()
    again = engine.ReadLengths.parse(world.text, chunk_bytes=MIDDLE)
    assert again.stats() == before
    again.close()


@pytest.mark.parametrize('residue', [0, 1, 2, 3])
def test_line_count_residues(residue):
    """A short text per residue of the line count mod 4, with and without
    its final LF, in one chunk and in several"""
    rng = np.random.default_rng(100 + residue)
    body = b''.join(fe.record(b'r%d' % k, int(rng.integers(0, 400)), rng) for k in range(30))
    body += b''.join([b'@tail\n', b'ACGTACGTACGTA\n', b'+\n'][:residue])
    assert body.count(b'\n') % 4 == residue and len(body) > 4 * 1024
    for text in (body, body[:-1]):
        want = fe.figures(fe.read_lengths(text))
        for chunk in (1024, 0):
            r = engine.ReadLengths.parse(text, chunk_bytes=chunk)
            assert r.stats() == {k: want[k] for k in fe.KEYS}, (len(text), chunk)
            r.close()


def _tool(path, capfdbinary, **kw):
    exc = None
    try:
        genome_tools.fqstats(path, **kw)
    except Exception as e:  # noqa: BLE001
        exc = type(e).__name__
    return capfdbinary.readouterr().out.decode('latin-1'), exc


def _file(data, tmp_path):
    path = str(tmp_path / 'reads.fastq')
    with open(path, 'wb') as fh:
        fh.write(data)
    return path


def test_empty_sequence_lines_only(tmp_path, capfdbinary):
    data = CASES['empty_sequences_only']['text'].encode('latin-1')
    r = engine.ReadLengths.parse(data)
    s = r.stats()
    assert (s['reads'], s['bases'], s['median']) == (3, 0, 0)
    assert s['n25'] is None and s['n50'] is None and s['n75'] is None
    lengths, counts = r.histogram()
    assert lengths.tolist() == [0] and counts.tolist() == [3]
    r.close()
    out, exc = _tool(_file(data, tmp_path), capfdbinary)
    assert exc is None and out.endswith('n25=False\nn50=False\nn75=False\n')


@pytest.mark.parametrize('data', [b'', b'@only\n', b'@only', b'\n'])
def test_no_reads_raise_and_print_nothing(data, tmp_path, capfdbinary):
    r = engine.ReadLengths.parse(data)
    assert (r.reads, r.bases) == (0, 0) and r.histogram()[0].size == 0
    r.close()
    for native in ('True', 'False'):
        assert _tool(_file(data, tmp_path), capfdbinary, native=native) == ('', 'ZeroDivisionError')


@pytest.mark.parametrize('name', NAMES)
def test_goldens_in_a_process_of_their_own(name, tmp_path):
    """The command line prints the reference's bytes, or ends as it does"""
    case = CASES[name]
    path = _file(case['text'].encode('latin-1'), tmp_path)
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get('PYTHONPATH', ''))
    res = subprocess.run([sys.executable, '-m', 'magot_amd.genome_tools', 'fqstats', path],
                         stdout=subprocess.PIPE, stderr=subprocess.PIPE, env=env, timeout=300)
    assert res.stdout == case['out'].encode('latin-1')
    if case['exc'] is None:
        assert res.returncode == 0, res.stderr[-2000:]
    else:
        assert res.returncode != 0 and case['exc'].encode() in res.stderr


@pytest.mark.parametrize('name', NAMES)
def test_goldens_on_both_paths(name, tmp_path, capfdbinary):
    case = CASES[name]
    path = _file(case['text'].encode('latin-1'), tmp_path)
    assert _tool(path, capfdbinary) == (case['out'], case['exc'])
    assert genome_tools.fqstats.last_path == ('fqstats', 'native', None)
    assert _tool(path, capfdbinary, native='False') == (case['out'], case['exc'])
    assert genome_tools.fqstats.last_path == ('fqstats', 'host', "native != 'True'")


def test_whole_text_through_the_tool(world, tmp_path, capfdbinary):
    path = _file(world.text, tmp_path)
    out, exc = _tool(path, capfdbinary)
    assert (out, exc) == (fe.text_of(world.figures), None)
