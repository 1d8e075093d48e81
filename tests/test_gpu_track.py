"""position_dic's bit track on the device (engine.GenomeTrack, track.hip)
against numpy (track_expect) and, through genome.position_dic and
genome_tools.at_content_from_fasta, against the reference's own results in
tests/golden/position_dic.json.  Shapes are the smallest that reach every
path: contigs at every word phase, shorter than a word and longer than many
rank blocks, windows around the word and block sizes, more than one block of
every kernel."""

import json
import math
import os
import subprocess
import sys

import numpy as np
import pytest

import track_expect as te
from magot_amd import _lib, engine, genome, genome_tools

pytestmark = pytest.mark.gpu

# test_gpu_mask.py's alphabet: both cases of acgtn, IUPAC, '-', '*', digits,
# the bytes next to the letter ranges, bytes >= 0x80
ALPHABET = np.frombuffer(b'acgtnACGTNryswkmbdhvRYSWKMBDHV-*0189@[`{ zZaA\x80\xc1\xe1\xfa\xff', np.uint8)
LENGTHS = [1, 31, 32, 33, 64, 95, 261, 4100, 70000]
ORIGIN = 64
BLOCK = 512  # bases per rank directory block

GOLD = te.load()
CASES = {c['name']: c for c in GOLD['cases']}
CACHE = {}


class World(object):
    def __init__(self):
        rng = np.random.default_rng(20261019)
        self.contigs = [('n%d' % n, ALPHABET[rng.integers(0, len(ALPHABET), n)].tobytes())
                        for n in LENGTHS]
        every = np.concatenate([np.roll(np.arange(256, dtype=np.uint8), 7 * k) for k in range(3)])
        self.contigs.append(('every_byte', every.tobytes()))
        self.names = [nm for nm, _ in self.contigs]
        self.lengths = [len(s) for _, s in self.contigs]
        self.base = (ORIGIN + np.concatenate([[0], np.cumsum(self.lengths)])).astype(np.int64)
        self.dev = engine.DeviceGenome(self.contigs)
        self.big = self.names.index('n70000')
        self.rng = np.random.default_rng(5)

    def words(self, arrays, n_words):
        """The plane for one bool array per contig: zero outside the contigs."""
        bits = np.zeros(n_words * 32, bool)
        for c, arr in enumerate(arrays):
            bits[self.base[c]:self.base[c] + self.lengths[c]] = arr
        return np.packbits(bits, bitorder='little').view('<u4')

    def zeros(self):
        return [np.zeros(n, bool) for n in self.lengths]

    def random(self, density=0.5):
        return [self.rng.random(n) < density for n in self.lengths]

    def track(self, arrays=None):
        t = engine.GenomeTrack(self.dev)
        if arrays is not None:
            for c, arr in enumerate(arrays):
                t.set_bytes(c, arr)
        return t


@pytest.fixture(scope='module')
def world():
    w = World()
    assert w.dev.handle and len({int(b) % 32 for b in w.base[:-1]}) == 5  # word phases differ
    assert int(_lib.lib().magot_track_rank_block()) == BLOCK
    yield w
    w.dev.close()


def same_words(got, want):
    bad = np.flatnonzero(got != want)
    assert len(bad) == 0, 'word %d: %08x, expected %08x' % (bad[0], got[bad[0]], want[bad[0]])


def test_a_new_track_is_zero_and_spans_the_genome(world):
    t = world.track()
    try:
        assert t.n_words * 32 >= world.base[-1] + 64
        assert not t.words().any()
    finally:
        t.close()


@pytest.mark.parametrize('gc', [False, True])
def test_base_class_planes(world, gc):
    want = [te.base_class(s, gc) for _, s in world.contigs]
    t = world.track()
    try:
        t.base_class(gc=gc, replace=True)
        same_words(t.words(), world.words(want, t.n_words))  # and zero outside the contigs
        t.base_class(gc=not gc, replace=True)  # replaces: nothing of the first class stays
        other = [te.base_class(s, not gc) for _, s in world.contigs]
        same_words(t.words(), world.words(other, t.n_words))
        t.base_class(gc=gc)  # OR: both classes
        same_words(t.words(), world.words([a | b for a, b in zip(want, other)], t.n_words))
        for c, arr in enumerate(want):
            assert np.array_equal(t.get_bytes(c), arr | other[c])
    finally:
        t.close()


def test_base_class_or_over_a_painted_track(world):
    had = world.random(0.3)
    t = world.track(had)
    try:
        t.base_class()
        want = [h | te.base_class(s) for h, (_, s) in zip(had, world.contigs)]
        same_words(t.words(), world.words(want, t.n_words))
    finally:
        t.close()


def paint_sets(w):
    """name -> (contig, start, length) rows; `a` is a base of the long contig
    at bit 0 of a word."""
    big = w.big
    a = int(64 + (-(w.base[big] + 64)) % 32)
    assert (w.base[big] + a) % 32 == 0
    b = lambda s, n: (big, a + s, n)  # noqa: E731
    return {
        'inside_one_word': [b(3, 7)],
        'ends_at_bit_31': [b(20, 12)],
        'starts_at_bit_0': [b(32, 9)],
        'spanning_words': [b(5, 101), b(300, 32 * 40 + 3)],
        'whole_words': [b(0, 32), b(64, 64)],
        'overlapping_nested_duplicate': [b(5, 66), b(5, 66), b(10, 11), b(71, 10), b(60, 40),
                                         b(0, 32 * 6), b(40, 5), b(64, 1), b(95, 1)],
        'whole_contigs': [(c, 0, n) for c, n in enumerate(w.lengths)],
        'longer_than_a_piece': [(big, 17, 69000), (big - 1, 1, 4098)],
        'first_and_last_bases': [(c, 0, 1) for c in range(len(w.lengths))] +
                                [(c, n - 1, 1) for c, n in enumerate(w.lengths)],
        'nothing': [],
    }


PAINT_SETS = ['inside_one_word', 'ends_at_bit_31', 'starts_at_bit_0', 'spanning_words',
              'whole_words', 'overlapping_nested_duplicate', 'whole_contigs',
              'longer_than_a_piece', 'first_and_last_bases', 'nothing']


@pytest.mark.parametrize('name', PAINT_SETS)
@pytest.mark.parametrize('value', [1, 0])
def test_paint(world, name, value):
    sets = paint_sets(world)
    assert sorted(sets) == sorted(PAINT_SETS)
    rows = sets[name]
    had = world.random(0.5) if PAINT_SETS.index(name) % 2 else \
        [np.full(n, value == 0) for n in world.lengths]
    want = [h.copy() for h in had]
    for c, s, n in rows:
        want[c][s:s + n] = bool(value)
    t = world.track(had)
    try:
        t.paint([r[0] for r in rows], [r[1] for r in rows], [r[2] for r in rows], value)
        same_words(t.words(), world.words(want, t.n_words))
    finally:
        t.close()


def test_bytes_round_trip_at_every_length(world):
    arrays = world.random(0.5)
    t = world.track()
    try:
        order = [3, 0, 9, 8, 1, 7, 2, 6, 5, 4]
        for c in order:  # each contig leaves its neighbours' bits alone
            t.set_bytes(c, arrays[c])
        same_words(t.words(), world.words(arrays, t.n_words))
        for c in order:
            got = t.get_bytes(c)
            assert got.dtype == bool and np.array_equal(got, arrays[c])
        # any non-zero byte sets the bit; the bytes that come back are 0 and 1
        for c in (1, 5, 8):
            raw = world.rng.choice(np.array([0, 0, 1, 2, 128, 255], np.uint8), world.lengths[c])
            t.set_bytes(c, raw)
            arrays[c] = raw != 0
            back = np.empty(world.lengths[c], np.uint8)
            t.get_bytes(c, out=back)
            assert np.array_equal(back, (raw != 0).astype(np.uint8))
        same_words(t.words(), world.words(arrays, t.n_words))
        with pytest.raises(_lib.MagotError):
            t.set_bytes(2, np.zeros(31, bool))
    finally:
        t.close()


def rank_tracks(w):
    ones = [np.ones(n, bool) for n in w.lengths]
    alt = [np.arange(n) % 2 == 1 for n in w.lengths]
    first, last = w.zeros(), w.zeros()
    first[w.big][0] = True
    last[w.big][-1] = True
    return {'ones': ones, 'zeros': w.zeros(), 'alternating': alt, 'first_base': first,
            'last_base': last}


@pytest.mark.parametrize('name', ['ones', 'zeros', 'alternating', 'first_base', 'last_base'])
def test_rank_and_count(world, name):
    arrays = rank_tracks(world)[name]
    big, n_big = world.big, world.lengths[world.big]
    to_block = int(-world.base[big] % BLOCK)  # the long contig's first block boundary
    to_word = int(-world.base[big] % 32)
    rows = [(c, 0, n) for c, n in enumerate(world.lengths)]                 # whole contigs
    rows += [(c, 0, 1) for c in range(len(world.lengths))]                  # length 1
    rows += [(c, n - 1, 1) for c, n in enumerate(world.lengths)]
    rows += [(big, to_word + 32 * k, 32 * m) for k, m in ((0, 1), (3, 2), (100, 17))]
    rows += [(big, to_block - 1, 2), (big, to_block - 33, 70), (big, to_block + BLOCK - 5, 1500),
             (big, to_block, BLOCK), (big, to_block, 40 * BLOCK), (big, 1, n_big - 2),
             (big, n_big - 1, 1), (big, 5, 0)]
    t = world.track(arrays)
    try:
        got = t.count([r[0] for r in rows], [r[1] for r in rows], [r[2] for r in rows])
        want = [int(arrays[c][s:s + n].sum()) for c, s, n in rows]
        assert got.tolist() == want
        t.paint([big], [7], [3], 1)  # a producer after a count: the directory is rebuilt
        arrays[big][7:10] = True
        assert t.count([big, 0], [0, 0], [n_big, 1]).tolist() == [int(arrays[big].sum()),
                                                                 int(arrays[0][0])]
    finally:
        t.close()


WINDOWS = [1, 2, 31, 32, 33, 63, 64, 65, 500, 4099, 69999]
JUMPS = [1, 3, 32, 997, 70001]


@pytest.fixture(scope='module')
def dense(world):
    """A track of runs: long stretches of ones and zeros and noisy parts, so
    that threshold tests flip often and rarely."""
    rng = np.random.default_rng(17)
    arrays = []
    for n in world.lengths:
        level = np.repeat(rng.random(n // 50 + 1), 50)[:n]
        arrays.append(rng.random(n) < level)
    t = world.track(arrays)
    yield t, arrays
    t.close()


def expected_windows(world, arrays, window, jump, skip):
    first, sums = [0], []
    for c, arr in enumerate(arrays):
        s = te.window_sums(arr, window, jump) if not skip[c] else np.zeros(0, np.int64)
        sums.append(s)
        first.append(first[-1] + len(s))
    return first, sums


@pytest.mark.parametrize('jump', JUMPS)
@pytest.mark.parametrize('window', WINDOWS)
def test_windows(world, dense, window, jump):
    t, arrays = dense
    for skip in ([False] * len(arrays), [c in (4, 8) for c in range(len(arrays))]):
        first, sums = expected_windows(world, arrays, window, jump, skip)
        w = t.windows(window, jump, skip=skip if any(skip) else None)
        try:
            assert w.first.tolist() == first and w.n_windows == first[-1]
            got = w.sums()
            assert got.dtype == np.uint32 and np.array_equal(got, np.concatenate(sums))
        finally:
            w.close()


@pytest.mark.parametrize('window,jump', [(1, 1), (33, 1), (64, 3), (500, 1), (500, 32),
                                         (4099, 1), (31, 997)])
def test_transitions(world, dense, window, jump):
    t, arrays = dense
    skip = [False] * len(arrays)
    first, sums = expected_windows(world, arrays, window, jump, skip)
    w = t.windows(window, jump)
    try:
        for s_min in (0, window + 1, 1, max(1, window // 2), max(1, (3 * window) // 4), window):
            got = w.transitions(s_min).astype(np.int64)
            want = [te.flips_of(s >= s_min) + first[c] for c, s in enumerate(sums)]
            assert np.array_equal(got, np.concatenate(want)), s_min
            cut = np.searchsorted(got, first)
            for c, s in enumerate(sums):
                flips = got[cut[c]:cut[c + 1]] - first[c]
                assert te.regions_from_flips(flips, window, jump, len(arrays[c])) == \
                    te.regions_walk(s >= s_min, window, jump, len(arrays[c])), (s_min, c)
    finally:
        w.close()


def test_device_resident_chain(world):
    """genome -> A/T class -> windows -> transitions without a per-base copy."""
    t = world.track()
    try:
        t.base_class()
        w = t.windows(100, 10)
        try:
            at = [te.base_class(s) for _, s in world.contigs]
            first, sums = expected_windows(world, at, 100, 10, [False] * len(at))
            want = [te.flips_of(s >= 20) + first[c] for c, s in enumerate(sums)]
            assert np.array_equal(w.transitions(20).astype(np.int64), np.concatenate(want))
        finally:
            w.close()
    finally:
        t.close()


def recorded(case):
    keys = ('stdout', 'stdout_sha', 'stdout_n', 'exc', 'result', 'arrays')
    return {k: case[k] for k in keys if k in case}


@pytest.mark.parametrize('name', sorted(CASES))
def test_goldens_through_the_device_path(name):
    """The device path takes exactly the calls it must, and either path gives
    the reference's values, regions, exceptions and printed lines."""
    case = CASES[name]
    pd, res, exc, out = te.run_case(genome, case, GOLD['genomes'], CACHE, native=True)
    assert json.loads(json.dumps(te.outcome(pd, res, exc, out))) == recorded(case)
    if case['decline'] is None:
        assert pd.last_path[1:] == ('native', None), pd.last_path
    else:
        assert pd.last_path[1] == 'host' and pd.last_path[2], case['decline']


NATIVE_DECLINES = {
    'gt_inside_a_line': b'>a x\nACGT\nAC>GT\nTTTT\n',
    'empty_record': b'>a\n>b\nacgtn\n',
    'repeated_name': b'>a\nAT\n>a\nGGC\n',
    'sequence_first': b'ACGT\n>a\nAC\n',
    'blank_then_header': b'\n>a\nAC\n',
    'empty_file': b'',
}


@pytest.mark.parametrize('name', sorted(NATIVE_DECLINES))
def test_at_content_from_fasta_declines(name, tmp_path):
    path = str(tmp_path / 'in.fa')
    with open(path, 'wb') as fh:
        fh.write(NATIVE_DECLINES[name])
    assert genome_tools._at_content_native(path, genome_tools._Clock()) is None


def test_at_content_from_fasta_native_small(tmp_path):
    data = b'>a one\r\nACGTNN\r\n\n\r\nacgu\r\n>b\r\nGG\n>c c\nnnRYKM-*\nATat\n'
    path = str(tmp_path / 'in.fa')
    with open(path, 'wb') as fh:
        fh.write(data)
    text = genome_tools._at_content_native(path, genome_tools._Clock())
    assert text == te.at_content_lines(data) == b'a one\t3\t4\nb\t0\t2\nc c\t4\t0\n'


def test_cli_child_process(golden_dir):
    """The tool in a process of its own on the O.biroi FASTA: the line loop's
    text, from the device path."""
    path = os.path.join(golden_dir, te.OBIROI_FA)
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, MAGOT_CLI_TIMING='1',
               PYTHONPATH=root + os.pathsep + os.environ.get('PYTHONPATH', ''))
    res = subprocess.run([sys.executable, '-m', 'magot_amd.genome_tools', 'at_content_from_fasta',
                          path], stdout=subprocess.PIPE, stderr=subprocess.PIPE, env=env,
                         timeout=300)
    assert res.returncode == 0, res.stderr[-2000:]
    with open(path, 'rb') as fh:
        assert res.stdout == te.at_content_lines(fh.read())
    phases = json.loads(res.stderr.decode().strip().splitlines()[-1])['cli_phases_s']
    assert 'kernels' in phases


def test_bad_arguments_are_refused_before_any_launch(world):
    arrays = world.random(0.5)
    t = world.track(arrays)
    other = engine.DeviceGenome([('x', b'ACGT' * 50)])
    try:
        before = t.words().copy()
        for window, jump in ((0, 1), (5, 0), (0, 0)):
            with pytest.raises(_lib.MagotError, match='at least 1'):
                t.windows(window, jump)
        big, n = world.big, world.lengths[world.big]
        for rows in ([(big, n - 3, 4)], [(0, 0, 1), (0, 1, 1)], [(len(arrays), 0, 1)],
                     [(big, 2 ** 32 - 2, 5)]):
            cols = [[r[k] for r in rows] for k in range(3)]
            with pytest.raises(_lib.MagotError, match='outside its contig'):
                t.paint_rows(engine._interval_rows(*cols), 1)
            with pytest.raises(_lib.MagotError, match='outside its contig'):
                t.count(*cols)
        with pytest.raises(_lib.MagotError, match='longer than one piece'):
            t.paint_rows(engine._interval_rows([big], [0], [t.piece + 1]), 1)
        with pytest.raises(_lib.MagotError, match='0 or 1'):
            t.paint([big], [0], [4], 2)
        with pytest.raises(_lib.MagotError, match='another genome'):
            t.base_class(genome=other)
        same_words(t.words(), before)
    finally:
        t.close()
        other.close()


def test_timing_entry_point(world, dense):
    t, _ = dense
    w = t.windows(500, 3)
    try:
        ms = t.time(2, windows=w, s_min=250)
        assert sorted(ms) == ['class', 'count', 'rank', 'transitions', 'windows']
        assert all(math.isfinite(v) and v > 0 for v in ms.values()), ms
        ms = t.time(1)
        assert ms['class'] > 0 and ms['rank'] > 0 and ms['count'] > 0
    finally:
        w.close()
