"""depth_from_gff's integer track on the device (engine.DepthTrack, depth.hip)
against the table generator's own arrays and numpy prefix sums, and, through
genome_tools.depth_from_gff, against the reference's own output in
tests/golden/depth_from_gff.json.  Shapes are the smallest that reach every
path: runs around the wave and the directory block sizes and one of many text
blocks, chunks of 4 KB (hundreds of seams), 64 KB and the default, a run head
that is a chunk's first line at each size, every class of offending line at a
table's and a chunk's first and last line.

Not reachable by a test of this size: a table of more than 2^31-1 lines.  The
run limit is met through ``max_runs``."""

import json
import os
import subprocess
import sys

import numpy as np
import pytest

import depth_expect as de
from magot_amd import _lib, engine, genome_tools

pytestmark = pytest.mark.gpu

B = 256  # depths per directory block
RUN_LENGTHS = [1, 2, 63, 64, 65, B - 1, B, B + 1, 4000, 70000, 3]
NAMES = ['a', 'N' * 255, 'c1', 'c10', 'c1x', 'r.6', 'r|7', 'r~8', 'mid', 'big', 'z']
SMALL, MIDDLE = 4096, 65536
INT_MAX = 2 ** 31 - 1

GOLD = de.load()
CASES = GOLD['cases']
RUNS = [(name, i) for name in sorted(CASES) for i in range(len(CASES[name]['runs']))]


def cuts(text, chunk):
    """Where the chunks start: each the longest piece of at most ``chunk``
    bytes that ends after an LF (the upload's rule, restated)."""
    out, off = [], 0
    while off < len(text):
        out.append(off)
        end = min(off + chunk, len(text))
        if end < len(text):
            end = text.rindex(b'\n', off, end) + 1
        off = end
    return out


def _line(name, pos, depth, i):
    """One line of the grammar, its optional parts chosen by the line's index."""
    sep = b' \t ' if i % 5 == 2 else b'\t'
    p = b'%d' % pos if i % 13 != 5 else b'000%d' % pos
    d = b'%d' % depth if i % 17 != 6 else b'%010d' % depth  # ten digits at the most
    extra = b'\tx  y' if i % 11 == 4 else b''
    tail = b' ' if i % 19 == 7 else b''
    return name + sep + p + sep + d + extra + tail + (b'\r\n' if i % 7 == 3 else b'\n')


def _pad_to(lines, need, per_line):
    """Fourth columns on plain lines (and one leading zero) until they have
    ``need`` more bytes; no line grows by more than per_line + 1."""
    assert 0 <= need <= len(lines) * per_line
    k = 0
    while need:
        step = need if need <= per_line + 1 and need != 1 else min(need, per_line)
        if need - step == 1:
            step -= 1
        head, _, depth = lines[k][:-1].rpartition(b'\t')
        if step == 1 and len(depth) > 9:  # ten digits at the most: the next line
            k += 1
            continue
        if step == 1:  # a leading zero on the depth
            lines[k] = head + b'\t0' + depth + b'\n'
        else:
            lines[k] = lines[k][:-1] + b'\t' + b'p' * (step - 1) + b'\n'
        need -= step
        k += 1


class World(object):
    """One table: the runs of RUN_LENGTHS, run 'c1x' ending at byte 4096 and
    run 'mid' at byte 65536 (the next run's head is then a chunk's first line
    at that chunk size), the last line without LF."""

    def __init__(self):
        rng = np.random.default_rng(20261019)
        self.arrays = []
        for n in RUN_LENGTHS:
            d = rng.integers(0, 1000, n).astype(np.int64)
            d[rng.integers(0, n, max(1, n // 50))] = 0
            d[rng.integers(0, n, max(1, n // 50))] = INT_MAX
            self.arrays.append(d)
        runs, i = [], 0
        for r, (nm, d) in enumerate(zip(NAMES, self.arrays)):
            plain = nm in ('c1', 'c10', 'c1x', 'mid')  # the lines that take the padding
            lines = []
            for pos, depth in enumerate(d.tolist(), 1):
                lines.append(_line(nm.encode(), pos, depth, 0 if plain else i))
                i += 1
            runs.append(lines)
        size = lambda rs: sum(len(ln) for r in rs for ln in r)  # noqa: E731
        pad = runs[2] + runs[3] + runs[4]
        _pad_to(pad, SMALL - size(runs[:5]), 16)
        runs[2], runs[3], runs[4] = pad[:63], pad[63:127], pad[127:]
        _pad_to(runs[8], MIDDLE - size(runs[:9]), 8)
        chunks = [b''.join(lines) for lines in runs]
        self.heads = np.concatenate([[0], np.cumsum([len(c) for c in chunks])])[:-1].tolist()
        self.text = b''.join(chunks)[:-1]  # the last line lacks its LF
        self.first = np.concatenate([[0], np.cumsum(RUN_LENGTHS)]).astype(np.int64)
        self.tracks = {}

    def track(self, chunk):
        if chunk not in self.tracks:
            self.tracks[chunk] = engine.DepthTrack.parse(self.text, chunk_bytes=chunk)
        return self.tracks[chunk]


@pytest.fixture(scope='module')
def world():
    w = World()
    assert int(_lib.lib().magot_depth_block()) == B
    # a run head is a chunk's first line at both sizes, CRLF and columns occur
    assert w.heads[5] == SMALL and cuts(w.text, SMALL)[1] == SMALL
    assert w.heads[9] == MIDDLE and cuts(w.text, MIDDLE)[1] == MIDDLE
    assert len(cuts(w.text, SMALL)) > 200 and len(cuts(w.text, MIDDLE)) > 10
    assert b'\r\n' in w.text and b'\tx  y' in w.text and b' \t ' in w.text and b'\t000' in w.text
    assert not w.text.endswith(b'\n')
    yield w
    for t in w.tracks.values():
        t.close()


@pytest.mark.parametrize('chunk', [SMALL, MIDDLE, None])
def test_parse_equals_the_generator(world, chunk):
    t = world.track(chunk)
    assert t.declined is None
    assert t.names == NAMES
    assert t.lengths.tolist() == RUN_LENGTHS and t.first.tolist() == world.first[:-1].tolist()
    assert t.n_lines == sum(RUN_LENGTHS)
    for c, want in enumerate(world.arrays):
        got = t.values(c)
        assert got.dtype == np.int32
        bad = np.flatnonzero(got != want)
        assert bad.size == 0, (chunk, NAMES[c][:8], bad[:5], got[bad[:5]], want[bad[:5]])
    assert (t.values('c10') == world.arrays[3]).all()


# -- declines ---------------------------------------------------------------

def _good(k, name=b'c1'):
    return name + b'\t%05d\t%06d\n' % (k + 1, (7 * k) % 13)  # 16 bytes for c1


OFFENDERS = [
    ('empty line', lambda k: b'\n'),
    ('empty line', lambda k: b'\r\n'),
    ('fewer than three fields', lambda k: b'c1\t%d\n' % (k + 1)),
    ('fewer than three fields', lambda k: b'c1 \n'),
    ('leading blank', lambda k: b' c1\t%d\t5\n' % (k + 1)),
    ('leading blank', lambda k: b'\t\n'),
    ('sign on a number', lambda k: b'c1\t+%d\t5\n' % (k + 1)),
    ('sign on a number', lambda k: b'c1\t%d\t-5\n' % (k + 1)),
    ('byte outside the grammar', lambda k: b'c1\t%d\t5\xe9\n' % (k + 1)),
    ('byte outside the grammar', lambda k: b'c\x80\t%d\t5\n' % (k + 1)),
    ('byte outside the grammar', lambda k: b'c1\t%d\t5\t\x01\n' % (k + 1)),
    ('byte outside the grammar', lambda k: b'c1\t%d\t5\rx\n' % (k + 1)),
    ('byte outside the grammar', lambda k: b'c1\x0b%d\t5\n' % (k + 1)),
    ('not a number', lambda k: b'c1\t%d\t5x\n' % (k + 1)),
    ('not a number', lambda k: b'c1\t%d.0\t5\n' % (k + 1)),
    ('number out of range', lambda k: b'c1\t%d\t12345678901\n' % (k + 1)),
    ('number out of range', lambda k: b'c1\t%d\t2147483648\n' % (k + 1)),
    ('number out of range', lambda k: b'c1\t00000000%03d\t5\n' % (k + 1)),
    ('name longer than 255 bytes', lambda k: b'N' * 256 + b'\t1\t5\n'),
    ('position out of sequence', lambda k: b'c1\t%d\t5\n' % (k + 3)),
    ('position out of sequence', lambda k: b'c1\t0\t5\n'),
    ('position out of sequence', lambda k: b'c2\t2\t5\n'),
]
N_LINES = 3 * SMALL // 16


def _table_with(bad, where):
    """(text, k): N_LINES lines of 16 bytes with line k replaced by bad(k);
    ``where``: the table's first or last line, or the first or last line of
    the second 4 KB chunk."""
    if where == 'first':
        k = 0
    elif where == 'last':
        k = N_LINES - 1
    elif where == 'chunk first':
        k = SMALL // 16
    else:  # the line that ends at byte 2 * SMALL: the one before it is padded
        b = len(bad(0))
        k = (2 * SMALL - b) // 16
        b = len(bad(k))
        k = (2 * SMALL - b) // 16
        if 2 * SMALL - b - 16 * k == 1:
            k -= 1
    lines = [_good(i) for i in range(N_LINES)]
    lines[k] = bad(k)
    if where == 'chunk last':
        rem = 2 * SMALL - len(lines[k]) - 16 * k
        if rem:
            lines[k - 1] = lines[k - 1][:-1] + b'\t' + b'p' * (rem - 1) + b'\n'
    return b''.join(lines), k


@pytest.mark.parametrize('where', ['first', 'last', 'chunk first', 'chunk last'])
def test_offending_lines_are_named(where):
    for reason, bad in OFFENDERS:
        text, k = _table_with(bad, where)
        starts = cuts(text, SMALL)
        at = sum(len(ln) for ln in text.split(b'\n')[:k]) + k
        if where == 'chunk first':
            assert at in starts[1:]
        elif where == 'chunk last':
            assert at + len(bad(k)) == 2 * SMALL and 2 * SMALL in starts
        for chunk in (SMALL, None):
            t = engine.DepthTrack.parse(text, chunk_bytes=chunk)
            try:
                assert t.declined == (reason, k + 1), (bad(k), where, chunk)
                assert t.handle is None and t.names == [] and t.n_lines == 0
            finally:
                t.close()


def test_repeated_contig_and_whole_table_limits():
    runs = [(b'c1', 300), (b'c2', 212), (b'c1', 5), (b'c3', 4)]
    text = b''.join(_good(i, nm) for nm, n in runs for i in range(n))
    assert cuts(text, SMALL)[2] == 512 * 16  # the repeated head is a chunk's first line
    for chunk in (SMALL, None):
        assert engine.DepthTrack.parse(text, chunk_bytes=chunk).declined == ('repeated contig', 513)
    # an offending line before the repeated head comes first, one after it does not
    early = text.replace(b'c1\t00007\t', b'c1\t00009\t', 1)
    assert engine.DepthTrack.parse(early, chunk_bytes=SMALL).declined == \
        ('position out of sequence', 7)
    late = text[:-1] + b'x\n'
    assert engine.DepthTrack.parse(late, chunk_bytes=SMALL).declined == ('repeated contig', 513)
    three = b''.join(_good(i, nm) for nm, n in [(b'c1', 3), (b'c2', 3), (b'c3', 3)] for i in range(n))
    t = engine.DepthTrack.parse(three, max_runs=3)
    assert t.declined is None and t.names == ['c1', 'c2', 'c3']
    t.close()
    assert engine.DepthTrack.parse(three, max_runs=2).declined == ('too many runs', None)
    long_line = _good(0) + b'c1\t2\t5\t' + b'x' * 5000 + b'\n' + _good(2)
    assert engine.DepthTrack.parse(long_line, chunk_bytes=SMALL).declined == \
        ('line longer than a chunk', 2)
    t = engine.DepthTrack.parse(long_line)  # one chunk: inside the grammar
    assert t.declined is None and t.values(0).tolist() == [0, 5, 1]
    t.close()
    empty = engine.DepthTrack.parse(b'')
    assert empty.declined is None and empty.names == [] and empty.n_lines == 0
    empty.close()


# -- sums -------------------------------------------------------------------

def _clip(length, a, b):
    lo, hi = slice(a, b).indices(length)[:2]
    return lo, max(0, hi - lo)


def test_sums_equal_numpy(world):
    t = world.track(None)
    big = NAMES.index('big')
    rows = []  # (contig, a, b) as slices of the contig's array
    for s_off in range(-3, 4):
        for e_off in range(-3, 4):
            rows.append((big, 5 * B + s_off, 9 * B + e_off))
            rows.append((big, 7 * B + s_off, 7 * B + e_off))  # inside one block, or empty
    for n in (0, 1, B, 3 * B + 1):
        for a in (0, 1, B - 1, B, B + 1, 70000 - n, 69990):
            rows.append((big, a, a + n))
    for c, n in enumerate(RUN_LENGTHS):
        rows += [(c, 0, n), (c, 0, n + 50), (c, n - 1, n), (c, n, n + 5), (c, n + 7, n + 9),
                 (c, n // 2, n // 3)]
    clipped = [(c,) + _clip(RUN_LENGTHS[c], a, b) for c, a, b in rows]
    tab = np.array(clipped, dtype=np.int64)
    want = np.array([world.arrays[c][a:b].sum() if b > a else 0 for c, a, b in rows], np.int64)
    got = t.sums(tab[:, 0], tab[:, 1], tab[:, 2])
    assert got.dtype == np.int64 and (got == want).all(), np.flatnonzero(got != want)[:5]
    assert want.max() > 2 ** 32  # sums leave 32 bits
    # negative and zero lengths give 0 wherever they start
    assert t.sums([0, big, 2], [0, 69999, 5], [-4, 0, -1]).tolist() == [0, 0, 0]
    # groups: one row, 300 rows, none
    rng = np.random.default_rng(7)
    a = rng.integers(0, 69000, 301)
    n = rng.integers(0, 900, 301)
    offsets = [0, 1, 301, 301]
    sums, groups = t.group_sums(np.full(301, big), a, n, offsets)
    each = np.array([world.arrays[big][x:x + k].sum() for x, k in zip(a.tolist(), n.tolist())])
    assert (sums == each).all()
    assert groups.tolist() == [int(each[0]), int(each[1:].sum()), 0]
    # a row outside the table is refused before any launch
    with pytest.raises(engine.MagotError):
        t.sums([NAMES.index('z')], [0], [4])
    with pytest.raises(engine.MagotError):
        t.group_sums([0], [0], [1], [0, 2])
    ms = t.time(1)
    assert set(ms) == {'line_index', 'parse', 'directory', 'sums', 'chunk_bytes'}
    assert ms['chunk_bytes'] == len(world.text) and ms['parse'] > 0
    assert (t.values(big) == world.arrays[big]).all()  # the timed passes change nothing
    for chunk, slot in ((SMALL, 0), (2 * MIDDLE, 1)):  # the last of many chunks, in either slot
        starts = cuts(world.text, chunk)
        assert len(starts) > 2 and (len(starts) - 1) % 2 == slot
        many = world.track(chunk)
        assert many.time(1)['chunk_bytes'] == len(world.text) - starts[-1]
        assert (many.values(big) == world.arrays[big]).all()


# -- the tool ---------------------------------------------------------------

def _tool(paths, run, order, capfdbinary, **kw):
    exc = None
    try:
        genome_tools.depth_from_gff(paths[0], paths[1], features=run['features'],
                                    stream_length=run['stream_length'], order=order, **kw)
    except Exception as e:  # noqa: BLE001
        exc = type(e).__name__
    return capfdbinary.readouterr().out, exc


@pytest.mark.parametrize('name,i', RUNS, ids=['%s-%d' % r for r in RUNS])
def test_goldens(name, i, tmp_path, capfdbinary):
    """The native path takes exactly the runs it must, for the recorded
    reason otherwise, and the tool prints the reference's bytes either way."""
    case = CASES[name]
    run = case['runs'][i]
    paths = de.case_files(case, tmp_path)
    if i == 0:
        with open(paths[0], 'rb') as fh:
            t = engine.DepthTrack.parse(fh.read(), chunk_bytes=1024)
        want = case['file_decline']
        assert t.declined == (None if want is None else tuple(want))
        t.close()
    for order in ('insertion', 'py2'):
        out, exc = _tool(paths, run, order, capfdbinary)
        de.same_as_recorded(out, exc, run[order])
        why = run[order]['decline']
        assert genome_tools.depth_from_gff.last_path == \
            ('depth_from_gff', 'native' if why is None else 'host', why)
    if 'depth_spec' in case:  # test_depth_host.py runs the loop over the large table
        return
    out, exc = _tool(paths, run, 'py2', capfdbinary, native='False')
    de.same_as_recorded(out, exc, run['py2'])
    assert genome_tools.depth_from_gff.last_path[1:] == ('host', "native != 'True'") or \
        run['py2']['exc'] == 'NameError'


def test_cli_in_a_process_of_its_own(tmp_path):
    case = CASES['example']
    run = case['runs'][1]
    dp, gp = de.case_files(case, tmp_path)
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, MAGOT_CLI_TIMING='1',
               PYTHONPATH=root + os.pathsep + os.environ.get('PYTHONPATH', ''))
    res = subprocess.run([sys.executable, '-m', 'magot_amd.genome_tools', 'depth_from_gff', dp, gp,
                          'stream_length=' + run['stream_length'], 'order=insertion'],
                         stdout=subprocess.PIPE, stderr=subprocess.PIPE, env=env, timeout=300)
    assert res.returncode == 0, res.stderr[-2000:]
    de.same_as_recorded(res.stdout, None, run['insertion'])
    phases = json.loads(res.stderr.decode().strip().splitlines()[-1])['cli_phases_s']
    assert 'kernels' in phases and 'depth_parse' in phases
