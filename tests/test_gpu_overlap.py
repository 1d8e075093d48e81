"""The interval joins on the device (overlap.hip; genome_tools.py:548-568,
annotation_funcs.py:13-30): engine.IntervalIndex against the reference's two
predicates as brute force over all pairs (overlap_expect.py), exactly; the
recorded runs of the reference through genome_tools.purge_overlaps and
annotation_funcs.annotation_overlap on both paths; one command-line call.

Index sizes: none, one, around a wave and around a workgroup, and 4000 (the
sorts then span several blocks); about 3000 queries each, so the brute force
stays near 10^7 pairs.  Range scans: none, one, and around the size at which a
wave takes over from a lane, and 1000."""

import os
import subprocess
import sys

import numpy as np
import pytest

import overlap_expect as oe
from magot_amd import annotation_funcs, engine, genome, genome_tools

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = oe.load()
PURGE = sorted(GOLD['purge'])
OVERLAP = sorted(GOLD['overlap'])
SIZES = [0, 1, 63, 64, 65, 255, 256, 257, 4000]


def test_the_constants_the_worlds_are_built_on():
    assert engine.IntervalIndex.coord_range() == (oe.COORD_LO, oe.COORD_HI)
    assert engine.IntervalIndex.lane_scan() == 64


@pytest.fixture(scope='module', params=SIZES)
def world(request):
    """An index of the given size, its queries and both brute-force answers"""
    index = oe.index_world(request.param)
    query = oe.query_world(*index)
    assert len(index[0]) == request.param and 2900 <= len(query[0]) <= 3100
    ix = engine.IntervalIndex(*index, n_seq=oe.N_SEQ)
    yield ix, query, oe.purge_brute(*index, *query), oe.overlap_brute(*index, *query)
    ix.close()


def test_purge_flags_equal_the_brute_force(world):
    ix, query, purge, _ = world
    got = ix.purge_flags(*query)
    assert got.dtype == bool and got.shape == purge.shape
    assert np.array_equal(got, purge), np.flatnonzero(got != purge)[:10]
    if ix.n >= 255:  # the world is not trivial: both answers occur, on several seqids
        assert len(set(query[0][purge])) >= 3 and len(set(query[0][~purge])) >= 5


def test_overlap_counts_equal_the_brute_force(world):
    ix, query, _, counts = world
    got = ix.overlap_counts(*query)
    assert got.dtype == np.int64 and got.shape == counts.shape
    assert np.array_equal(got, counts), np.flatnonzero(got != counts)[:10]
    if ix.n == 4000:  # some query's range goes to a wave, most stay with their lane
        assert counts.max() > 150 and (counts == 0).any()


def test_queries_may_repeat_and_be_empty(world):
    ix, query, purge, counts = world
    none = np.zeros(0, np.int64)
    assert ix.purge_flags(none, none, none).shape == (0,)
    assert ix.overlap_counts(none, none, none).shape == (0,)
    assert np.array_equal(ix.overlap_counts(*query), counts)  # the slot is reused
    assert np.array_equal(ix.purge_flags(*[c[:7] for c in query]), purge[:7])


def test_the_world_holds_the_edges_it_promises():
    seq, p0, p1 = oe.index_world(4000)
    assert {-5, 0, 1, 2} <= set((p1 - p0)[seq == 0].tolist())
    assert (p0[seq == 0] == 100).sum() >= 150 and (p1[seq == 0] == 200).sum() >= 150
    assert (seq == 1).sum() == 0 and (seq == 2).sum() == 1
    for s in (3, 4):
        assert p0[seq == s].min() == oe.COORD_LO and p1[seq == s].max() == oe.COORD_HI
    assert (p0 < 0).any() and set(oe.BIG) <= set(p0.tolist()) | set(p1.tolist())
    qseq, c0, c1 = oe.query_world(seq, p0, p1)
    assert (c0 > c1).any() and (c0 == c1).any() and set(oe.BIG) <= set(c0.tolist())
    assert {-1, 0, 1, 2, 3, 4, 5, oe.N_SEQ + 3} <= set(qseq.tolist())


SCAN = 64  # engine.IntervalIndex.lane_scan(), checked above
RANGES = [0, 1, SCAN - 1, SCAN, SCAN + 1, 1000]


def test_range_scans_on_both_sides_of_the_wave_threshold():
    index, query = oe.range_world(RANGES)
    # what each query's scan covers: the intervals that start in (1000, 5000]
    inside = [int(((index[0] == k) & (index[1] > 1000) & (index[1] <= 5000)).sum())
              for k in range(len(RANGES))]
    assert inside == RANGES
    want = oe.overlap_brute(*index, *query)
    ix = engine.IntervalIndex(*index)
    try:
        got = ix.overlap_counts(*query)
        assert np.array_equal(got, want), (got, want)
        assert np.array_equal(ix.purge_flags(*query), oe.purge_brute(*index, *query))
        # a query in the middle of many that take the other path
        seq, q0, q1 = oe.query_world(*index, n=600)
        seq, q0, q1 = (np.concatenate([a, b]) for a, b in zip((seq, q0, q1), query))
        assert np.array_equal(ix.overlap_counts(seq, q0, q1), oe.overlap_brute(*index, seq, q0, q1))
    finally:
        ix.close()


def test_arguments_are_checked_before_any_launch():
    with pytest.raises(engine.MagotError, match='coordinate outside'):
        engine.IntervalIndex([0], [oe.COORD_HI + 1], [5])
    with pytest.raises(engine.MagotError, match='coordinate outside'):
        engine.IntervalIndex([0], [5], [oe.COORD_LO - 1])
    with pytest.raises(ValueError):
        engine.IntervalIndex([-1], [1], [5])
    with pytest.raises(ValueError):
        engine.IntervalIndex([0, 0], [1], [5])
    ix = engine.IntervalIndex([0], [1], [5])
    try:
        with pytest.raises(engine.MagotError, match='coordinate outside'):
            ix.purge_flags([0], [oe.COORD_HI + 1], [0])
        with pytest.raises(engine.MagotError, match='coordinate outside'):
            ix.overlap_counts([0], [0], [oe.COORD_LO - 1])
        assert ix.purge_flags([0, 1, -1], [2, 2, 2], [3, 3, 3]).tolist() == [True, False, False]
    finally:
        ix.close()


def test_time_names_every_pass():
    index = oe.index_world(4000)
    ix = engine.IntervalIndex(*index, n_seq=oe.N_SEQ)
    try:
        t = ix.time(1)
        assert set(t) == set(engine.IntervalIndex.PASSES) | {'copy_bytes'}
        assert t['purge'] == 0 and t['overlap'] == 0 and t['sort'] > 0
        assert t['copy_bytes'] == 6 * 8 * 4000
        query = oe.query_world(*index)
        want = oe.overlap_brute(*index, *query)
        assert np.array_equal(ix.overlap_counts(*query), want)
        t = ix.time(2)
        assert t['purge'] > 0 and t['overlap'] > 0 and t['copy'] > 0
        # timing rebuilt the tables in place: the answers stand
        assert np.array_equal(ix.overlap_counts(*query), want)
        assert np.array_equal(ix.purge_flags(*query), oe.purge_brute(*index, *query))
    finally:
        ix.close()


# ---------------------------------------------------------------------------
# the recorded runs
# ---------------------------------------------------------------------------

def _files(case, tmp_path):
    paths = [str(tmp_path / 'first.gff'), str(tmp_path / 'second.gff')]
    for p, key in zip(paths, ('first', 'second')):
        with open(p, 'wb') as fh:
            fh.write(case[key].encode('latin-1'))
    return paths


def _purge(paths, capfdbinary, **kw):
    exc = None
    try:
        genome_tools.purge_overlaps(*paths, **kw)
    except Exception as e:  # noqa: BLE001
        exc = type(e).__name__
    return capfdbinary.readouterr().out.decode('latin-1'), exc


@pytest.mark.parametrize('name', PURGE)
def test_purge_goldens_on_both_paths(name, tmp_path, capfdbinary):
    case = GOLD['purge'][name]
    paths = _files(case, tmp_path)
    assert _purge(paths, capfdbinary) == (case['out'], case['exc'])
    why = None if case['path'] == 'native' else oe.REASONS[case['path']]
    assert genome_tools.purge_overlaps.last_path == \
        ('purge_overlaps', 'native' if why is None else 'host', why)
    assert _purge(paths, capfdbinary, native='False') == (case['out'], case['exc'])
    assert genome_tools.purge_overlaps.last_path == ('purge_overlaps', 'host', "native != 'True'")


@pytest.mark.parametrize('order', ['insertion', 'py2'])
@pytest.mark.parametrize('name', OVERLAP)
def test_overlap_goldens_on_both_paths(name, order):
    rec = GOLD['overlap'][name]
    for native in (True, False):
        d1 = oe.build_features(genome, rec['first'], rec['first_dict'])
        d2 = oe.build_features(genome, rec['second'], rec['second_dict'])
        res = exc = None
        try:
            res = annotation_funcs.annotation_overlap(d1, d2, order=order, native=native)
        except Exception as e:  # noqa: BLE001
            exc = type(e).__name__
        assert (res, exc) == (rec[order]['out'], rec[order]['exc'])
        path = annotation_funcs.annotation_overlap.last_path
        if not native:
            assert path == ('annotation_overlap', 'host', 'native is not True')
        elif name.startswith('childless_parent'):
            assert path == ('annotation_overlap', 'host', 'get_coords() is None or raises')
        else:
            assert path == ('annotation_overlap', 'native', None)


def test_a_larger_purge_through_the_tool(tmp_path, capfdbinary):
    """Some thousands of lines on five seqids, one of them absent from the first file"""
    rng = np.random.default_rng(20261023)

    def text(n, names):
        a = rng.integers(0, 200000, n)
        return b''.join(oe.gff_line(names[k % len(names)], int(x), int(x + w))
                        for k, (x, w) in enumerate(zip(a, rng.integers(-20, 400, n))))
    first, second = text(1500, ['c1', 'c2', 'c3', 'c4']), text(3000, ['c1', 'c2', 'c3', 'c4', 'c5'])
    want = oe.purge_expected(first, second)
    assert 0 < want.count(b'\n') < 3000
    paths = _files({'first': first.decode('latin-1'), 'second': second.decode('latin-1')}, tmp_path)
    assert _purge(paths, capfdbinary) == (want.decode('latin-1'), None)
    assert genome_tools.purge_overlaps.last_path[1] == 'native'


def test_the_command_line_in_a_process_of_its_own(tmp_path):
    case = GOLD['purge']['several_seqids']
    paths = _files(case, tmp_path)
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get('PYTHONPATH', ''))
    res = subprocess.run([sys.executable, '-m', 'magot_amd.genome_tools', 'purge_overlaps'] + paths,
                         stdout=subprocess.PIPE, stderr=subprocess.PIPE, env=env, timeout=300)
    assert res.returncode == 0, res.stderr[-2000:]
    assert res.stdout == case['out'].encode('latin-1')
