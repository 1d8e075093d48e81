"""orf6_kernel at its own edges: the builders of orf6_expect.py (what each holds
is asserted in test_orf6_edges_expect.py) through engine.orf6_batch (raw bytes)
and engine.Orf6Plan (the fused gather), against the expected buffer built from
the oracle's tables: the whole output [0, total) byte for byte, every stream at
its offset, zeros up to the next 16-byte boundary, nothing else.  The output is
filled with 0xEE before every launch, so a chunk that no lane wrote shows.

  (a) lengths  0..200, a first record of 3..47 bases, 1..21 records in a tile
  (b) seams    every phase of a seam in a stream, record ends at the seams
  (c) batches  1..400 records in a tile, 1,000 empty records, the tenth
               record's end at T1
  (d) chunks   1, 63, 64, 65, 128 chunks per strand; the bitmap's ranks
  (e) invalid  a non-ACGT byte at every window position and shift
  (f) fused    two-interval vectors, the exact path, 1..123 rows, the row cap,
               the only flagged row at 64..122, the contig's ends
  (g) order    genome order and MAGOT_ORF6_ORDER=record, empty records, equal keys"""

import numpy as np
import pytest

import orf6_expect as oe
from magot_amd import _lib, engine, shard
from test_tile_blocks import plan_debug

pytestmark = pytest.mark.gpu

POISON = 0xEE


def _batch(records):
    want, soff, slen = oe.expected(records)
    got, gsoff, gslen = engine.orf6_batch([r.tobytes() for r in records], poison=POISON, raw=True)
    assert np.array_equal(gsoff, soff) and np.array_equal(gslen, slen)
    msg = oe.first_difference(got, want, soff, slen)
    assert msg is None, msg


@pytest.fixture(scope='module')
def genome():
    dev = engine.DeviceGenome([('c0', oe.contig().tobytes())])
    yield dev
    dev.close()


def _plan(w, order, monkeypatch, dev=None):
    """w through ExtractionPlan + Orf6Plan in the given walk order: the stream
    table is the model's (and magot_orf6_sizes' in record order), the blocks
    tile the output, the bytes are the expected ones, twice."""
    if order == 'record':
        monkeypatch.setenv('MAGOT_ORF6_ORDER', 'record')
    else:
        monkeypatch.delenv('MAGOT_ORF6_ORDER', raising=False)
    records = w.record_bytes()
    ex_g = plan_debug([w.genome.tobytes()], w.ex, w.tx, _lib.OUT_NUC)['ex_g']
    perm = w.walk(ex_g, order)[0]
    want, soff, slen = oe.expected(records, perm)
    own = dev is None
    if own:
        dev = engine.DeviceGenome([('c0', w.genome.tobytes())])
    plan = o6 = None
    try:
        plan = engine.ExtractionPlan(dev, w.ex, w.tx, engine.OUT_NUC)
        o6 = engine.Orf6Plan(plan)
        assert o6.total == len(want)
        for again in range(2):
            o6.poison(POISON)
            if again == 0 and o6.total:     # the hook itself: nothing but the fill before a launch
                assert (o6.fetch()[0] == POISON).all()
            o6.execute()
            got, gsoff, gslen = o6.fetch()
            assert np.array_equal(gslen, slen) and np.array_equal(gsoff, soff)
            msg = oe.first_difference(got, want, soff, slen)
            assert msg is None, 'execute %d: %s' % (again, msg)
        if order == 'record':
            ref_soff, ref_slen = engine.orf6_sizes(np.array(oe.offsets(len(r) for r in records)))
            assert np.array_equal(gsoff, ref_soff) and np.array_equal(gslen, ref_slen)
        st, ln = shard.six_frame_blocks(gsoff, gslen)
        by = np.argsort(st, kind='stable')
        assert (st % 16 == 0).all() and int(gsoff[-1]) == o6.total
        if len(st):
            assert st[by][0] == 0 and int(st[by][-1] + ln[by][-1]) == o6.total
            assert np.array_equal(np.cumsum(ln[by])[:-1], st[by][1:])
    finally:
        for h in (o6, plan) + ((dev,) if own else ()):
            if h is not None:
                h.close()


# ---------------------------------------------------------------------------
# raw bytes: (a)-(e)
# ---------------------------------------------------------------------------

def test_every_length_through_the_batch():
    _batch(oe.lengths_all())


def test_a_short_first_record_through_the_batch():
    for L in oe.FIRST_LENGTHS:
        _batch(oe.lengths_first(L))


def test_record_counts_in_one_tile_through_the_batch():
    for n in oe.N_RECS:
        _batch(oe.lengths_n_rec(n))


def test_the_seams_through_the_batch():
    _batch(oe.seams())


def test_the_record_batches_through_the_batch():
    _batch(oe.batches())


@pytest.mark.parametrize('n', oe.PER_STRAND)
def test_the_chunk_passes_through_the_batch(n):
    _batch(oe.chunk_counts(n))


def test_the_bitmap_ranks_through_the_batch():
    _batch(oe.segment_bits())


@pytest.mark.parametrize('part', range(oe.INVALID_PARTS))
def test_invalid_bytes_through_the_batch(part):
    _batch(oe.invalid(part))


def test_the_batch_s_poison_is_off_by_default():
    recs = oe.raw_case([100, 0, 7], 11)
    want = oe.expected(recs)[0]
    got = engine.orf6_batch([r.tobytes() for r in recs], raw=True)[0]
    assert np.array_equal(got, want)
    six = engine.orf6_batch([r.tobytes() for r in recs])
    assert len(six) == 3 and six[1] == [None] * 6


# ---------------------------------------------------------------------------
# the fused gather: (a)-(c), (f), (g)
# ---------------------------------------------------------------------------

@pytest.mark.parametrize('order', oe.ORDERS)
@pytest.mark.parametrize('name', sorted(oe.RAW_OVER_PLAN))
def test_raw_builders_through_the_plan(monkeypatch, name, order):
    _plan(oe.over_genome(oe.RAW_OVER_PLAN[name]()), order, monkeypatch)


@pytest.mark.parametrize('order', oe.ORDERS)
@pytest.mark.parametrize('name', sorted(oe.FUSED))
def test_fused_builders_through_the_plan(monkeypatch, genome, name, order):
    _plan(oe.FUSED[name](), order, monkeypatch, genome)


@pytest.mark.parametrize('order', oe.ORDERS)
def test_every_row_count_through_the_plan(monkeypatch, genome, order):
    for m in oe.ROWS_STAGED:
        _plan(oe.fused_rows(m), order, monkeypatch, genome)


@pytest.mark.parametrize('order', oe.ORDERS)
def test_an_only_flagged_row_in_the_upper_lanes_through_the_plan(monkeypatch, genome, order):
    for k in oe.ONLY_FLAGGED:
        _plan(oe.fused_rows(oe.CAP, flagged=k), order, monkeypatch, genome)
