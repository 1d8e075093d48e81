"""The extraction planner (magot_amd/csrc/tileplan.cpp) on the CPU, through
magot_debug_tile_cut (the cut over given tables) and magot_debug_plan
(validation, compaction and flags, layout, cut, tile size, launch order).

Expected values are Python arithmetic on the definitions: the cut's model is
test_tile_blocks.cut, everything else is worked out here from the inputs.
"""

from bisect import bisect_right

import numpy as np
import pytest

from magot_amd import _lib
from test_tile_blocks import (BLK_EX, BLK_TX, CHUNK, EXC, EXON_CAP, FULL_TX_RECORDS, HALO, RC,
                              SLOWLIT, TX_CAP, const_exons, cut, find_length, full_exon_records,
                              layout, plan_debug, real_cut, single_exon, tile_bytes)

ORIGIN = 64  # pad bases before the first contig (kOrigin)
FLAGS = RC | EXC | SLOWLIT


# ---------------------------------------------------------------------------
# The cut
# ---------------------------------------------------------------------------

def seed7_records():
    rng = np.random.default_rng(7)
    return [[int(x) for x in rng.integers(1, 400, size=1 + rng.poisson(6))] for _ in range(600)]


def small_random_layouts():
    rng = np.random.default_rng(2024)
    return [[[int(x) for x in rng.integers(1, 301, size=rng.integers(1, 13))]
             for _ in range(rng.integers(1, 41))] for _ in range(200)]


def cut_cases(lc):
    """(name, records) of every layout the cut is checked on."""
    cases = [('seed7', seed7_records()), ('full_exon', full_exon_records()),
             ('full_tx', FULL_TX_RECORDS), ('threes', [[3]] * 200), ('one_tile', [[300]]),
             ('short_last_tile', FULL_TX_RECORDS[:48] + [[7]])]
    for want_m in (BLK_EX, BLK_EX + 1):
        L = find_length(const_exons(40, 150), lc, lambda m, nt: m == want_m, range(120, 8, -1))
        cases.append(('m=%d' % want_m, const_exons(40, 150)(L)))
    for want_nt in (BLK_TX - 1, BLK_TX):
        L = find_length(single_exon(1500), lc, lambda m, nt: nt == want_nt, range(600, 2, -3))
        cases.append(('nt=%d' % want_nt, single_exon(1500)(L)))
    cases += [('random%d' % i, r) for i, r in enumerate(small_random_layouts())]
    return cases


def check_tile_invariants(tiles, ex_out, tn, tp, lc):
    B, P, Tc = ex_out[-1], tp[-1], len(tn) - 1
    T0, T1, Q0, Q1 = (tiles[k].astype(np.int64) for k in ('T0', 'T1', 'Q0', 'Q1'))
    e1, e2, j1, j2 = (tiles[k].astype(np.int64) for k in ('e1', 'e2', 'j1', 'j2'))
    # the tiles partition [0, B) and [0, P), in order
    assert T0[0] == 0 and T1[-1] == B and np.array_equal(T1[:-1], T0[1:]) and (T1 > T0).all()
    assert Q0[0] == 0 and Q1[-1] == P and np.array_equal(Q1[:-1], Q0[1:]) and (Q1 >= Q0).all()
    assert (T1 - T0 <= tile_bytes(lc)).all()
    assert (e2 - e1 <= EXON_CAP).all() and (j2 - j1 <= TX_CAP - 1).all()
    assert not (T1[:-1] % CHUNK).any()
    for a, b, q0, q1 in zip(T0.tolist(), T1.tolist(), Q0.tolist(), Q1.tolist()):
        if q1 > q0:  # the last owned residue's codon lies in what the tile decodes
            j = bisect_right(tp, q1 - 1, 0, Tc) - 1
            assert tn[j] + 3 * (q1 - 1 - tp[j]) + 3 <= min(b + HALO, B)


@pytest.mark.parametrize('lc', [3, 6])
def test_cut_matches_model_and_invariants(lc):
    seen_m, seen_nt = set(), set()
    for name, recs in cut_cases(lc):
        ex_out, tn, tp = layout(recs)
        got = real_cut(ex_out, tn, tp, lc)
        want = cut(ex_out, tn, tp, lc)
        assert got.dtype == want.dtype
        assert np.array_equal(got, want), (name, lc)
        check_tile_invariants(got, ex_out, tn, tp, lc)
        seen_m |= set((got['e2'].astype(np.int64) - got['e1']).tolist())
        seen_nt |= set((got['j2'].astype(np.int64) - got['j1']).tolist())
        if name == 'one_tile':
            assert len(got) == 1
        if name == 'short_last_tile':
            assert int(got[-1]['T1']) - int(got[-1]['T0']) == 7
    # the boundary layouts stage what they were built for
    assert {BLK_EX, BLK_EX + 1, EXON_CAP} <= seen_m
    assert {BLK_TX - 1, BLK_TX, TX_CAP - 1} <= seen_nt


def test_cut_rejects_bad_lane_chunks():
    ex_out, tn, tp = (np.array(x, dtype=np.uint64) for x in layout([[300]]))
    n = np.zeros(1, dtype=np.uint64)
    rc = _lib.lib().magot_debug_tile_cut(_lib.ptr(ex_out), 1, _lib.ptr(tn), _lib.ptr(tp), 1, 4,
                                         None, 0, _lib.ptr(n))
    assert rc == _lib.ERR_ARG


# ---------------------------------------------------------------------------
# The whole planner: tables from (contig, start, length, reverse) intervals
# ---------------------------------------------------------------------------

def tables(recs):
    """(exons, txs) of records given as lists of (contig, start, len, reverse)."""
    ex = np.array([(start | (RC if rev else 0), ctg, n) for r in recs for ctg, start, n, rev in r],
                  dtype=_lib.EXON_DTYPE)
    tx = np.zeros(len(recs), dtype=_lib.TX_DTYPE)
    tx['n_exons'] = [len(r) for r in recs]
    tx['exon_begin'] = np.cumsum(tx['n_exons']) - tx['n_exons']
    return ex, tx


def acgt(rng, n):
    return np.frombuffer(b'ACGT', dtype=np.uint8)[rng.integers(0, 4, size=n)].copy()


@pytest.fixture(scope='module')
def genome3():
    """Three contigs of a few kilobases: an N run at [500, 520) of the second,
    one S (a byte without a literal class) at 300 of the third."""
    rng = np.random.default_rng(5)
    c = [acgt(rng, 2000), acgt(rng, 1500), acgt(rng, 1000)]
    c[1][500:520] = ord('N')
    c[2][300] = ord('S')
    return [x.tobytes() for x in c]


BASE3 = [ORIGIN, ORIGIN + 2000, ORIGIN + 3500]  # each contig's first global coordinate


@pytest.fixture
def no_overrides(monkeypatch):
    monkeypatch.delenv('MAGOT_EXTRACT_LANE_CHUNKS', raising=False)
    monkeypatch.delenv('MAGOT_TILE_BLOCK_ROWS', raising=False)


def plan_fails(contigs, ex, tx, status, text):
    with pytest.raises(_lib.MagotError) as err:
        plan_debug(contigs, ex, tx)
    assert '(status %d): magot_plan_create: %s' % (status, text) in str(err.value)


def test_validation_of_records(genome3):
    ex, tx = tables([[(0, 10, 30, False), (0, 50, 30, False)], [(1, 10, 30, True)],
                     [(2, 10, 30, False)]])
    plan_debug(genome3, ex, tx)  # the tables are good
    bad = tx.copy()
    bad['exon_begin'][1] = 1
    plan_fails(genome3, ex, bad, _lib.ERR_ARG,
               'record 1 does not start where the previous one ended')
    bad = tx.copy()
    bad['n_exons'][2] = 2
    plan_fails(genome3, ex, bad, _lib.ERR_ARG, 'records reference more exons than given')
    plan_fails(genome3, ex, tx[:2], _lib.ERR_ARG, 'exons not covered by records')


@pytest.mark.parametrize('which, exon', [('start', (1, 1501, 0, False)), ('end', (1, 1400, 101, True)),
                                         ('contig', (3, 0, 1, False))])
def test_validation_of_intervals(genome3, which, exon):
    recs = [[(0, 10, 30, False), (0, 50, 30, False)], [(1, 1400, 100, True), exon],
            [(2, 10, 30, False)]]
    ex, tx = tables(recs)
    plan_fails(genome3, ex, tx, _lib.ERR_RANGE, 'exon 3 outside its contig')
    recs[1][1] = (1, 1500, 0, False)  # an empty interval at the contig's end is inside it
    plan_debug(genome3, *tables(recs))


def test_validation_names_the_first_bad_interval_threaded(genome3, monkeypatch):
    """40 000 records: the count sweep runs on several threads, over the record
    ranges [0, 10000) ... [30000, 40000)."""
    monkeypatch.setenv('OMP_NUM_THREADS', '4')
    n = 40000
    ex = np.zeros(n, dtype=_lib.EXON_DTYPE)
    ex['start_rc'] = np.arange(n) % 1900
    ex['len'] = 50
    tx = np.zeros(n, dtype=_lib.TX_DTYPE)
    tx['exon_begin'] = np.arange(n)
    tx['n_exons'] = 1
    assert plan_debug(genome3, ex, tx)['B'] == 50 * n
    ex['start_rc'][15000] = 1951
    ex['contig'][n - 1] = 7
    plan_fails(genome3, ex, tx, _lib.ERR_RANGE, 'exon 15000 outside its contig')


def test_flags_and_compaction(genome3, no_overrides):
    # (interval, the flags it must get); zero-length intervals get no row
    rows = [((0, 100, 100, False), 0), ((0, 100, 100, True), 0),
            ((1, 0, 0, False), None),
            ((1, 490, 15, False), EXC), ((1, 510, 30, True), EXC),
            ((2, 290, 20, False), EXC | SLOWLIT), ((2, 290, 20, True), EXC),
            ((2, 300, 1, False), EXC | SLOWLIT), ((2, 0, 0, True), None),
            ((1, 400, 100, False), 0), ((1, 400, 100, True), 0),   # ends at the run's first base
            ((1, 520, 80, False), 0), ((1, 520, 80, True), 0),     # starts after its last
            ((2, 200, 100, False), 0), ((2, 301, 50, True), 0),
            ((1, 400, 101, False), EXC), ((1, 519, 81, True), EXC)]
    recs = [[r[0] for r in rows[:3]], [rows[3][0]], [r[0] for r in rows[4:9]], [rows[9][0]],
            [r[0] for r in rows[10:]]]
    plan = plan_debug(genome3, *tables(recs))
    kept = [(iv, fl) for iv, fl in rows if fl is not None]
    assert plan['Ec'] == len(kept) == len(rows) - 2
    want_g = [(BASE3[c] + s) | (RC if rev else 0) | fl for (c, s, n, rev), fl in kept]
    assert [int(x) for x in plan['ex_g'][:-1]] == want_g
    want_out = np.concatenate([[0], np.cumsum([iv[2] for iv, _ in kept])])
    assert np.array_equal(plan['ex_out'].astype(np.int64), want_out)
    assert plan['B'] == int(want_out[-1])
    rec_len = [sum(iv[2] for iv in r) for r in recs]
    assert plan['P'] == sum(n // 3 for n in rec_len)
    assert plan['Tc'] == len(recs)
    assert plan['tn'].tolist() == np.concatenate([[0], np.cumsum(rec_len)]).tolist()
    assert plan['tp'].tolist() == np.concatenate([[0], np.cumsum([n // 3 for n in rec_len])]).tolist()
    assert plan['lay_nuc'].tolist() == plan['tn'].tolist()[:-1]  # record order


def test_genome_order_layout(genome3, no_overrides):
    rng = np.random.default_rng(17)
    recs = []
    for ctg, start in [(2, 500), (0, 1200), (1, 30), (0, 40), (1, 30), (2, 10), (0, 900),
                       (1, 1000), (0, 40), (2, 700)]:
        lens = [int(x) for x in rng.integers(1, 60, size=3)]
        rev = bool(rng.integers(0, 2))
        # a leading empty interval does not place the record
        recs.append([(ctg, 0, 0, False), (ctg, start, lens[0], rev),
                     (ctg, start + 100, lens[1], rev), (ctg, start + 200, lens[2], rev)])
    recs.insert(3, [(1, 700, 0, False)])  # records without output
    recs.insert(8, [])
    ex, tx = tables(recs)
    plan = plan_debug(genome3, ex, tx, _lib.OUT_NUC | _lib.OUT_PEP | _lib.OUT_GENOME_ORDER)
    rec_len = [sum(iv[2] for iv in r) for r in recs]

    def key(t):
        first = [iv for iv in recs[t] if iv[2]]
        return BASE3[first[0][0]] + first[0][1] if first else 1 << 62
    order = sorted(range(len(recs)), key=key)  # stable: ties keep record order
    assert order[-2:] == [3, 8] and order.index(2) < order.index(5)  # (1, 30) twice
    want_nuc, want_pep, want_g, want_out = [0] * len(recs), [0] * len(recs), [], [0]
    acc = q = 0
    for t in order:
        want_nuc[t], want_pep[t] = acc, q
        acc += rec_len[t]
        q += rec_len[t] // 3
        for c, s, n, rev in recs[t]:
            if n:
                want_g.append((BASE3[c] + s) | (RC if rev else 0))
                want_out.append(want_out[-1] + n)
    assert plan['lay_nuc'].tolist() == want_nuc
    assert plan['lay_pep'].tolist() == want_pep
    assert [int(x) & ~(EXC | SLOWLIT) for x in plan['ex_g'][:-1]] == want_g
    assert plan['ex_out'].tolist() == want_out
    with_codon = [t for t in order if rec_len[t] >= 3]
    assert plan['tn'].tolist() == [want_nuc[t] for t in with_codon] + [acc]
    assert plan['tp'].tolist() == [want_pep[t] for t in with_codon] + [q]
    # the same tables in record order
    plain = plan_debug(genome3, ex, tx)
    assert plain['lay_nuc'].tolist() == np.concatenate([[0], np.cumsum(rec_len)])[:-1].tolist()
    assert (plain['B'], plain['P']) == (plan['B'], plan['P']) == (acc, q)


@pytest.fixture(scope='module')
def slow_workload():
    """300 forward records of three 200-base exons on one contig; an S inside
    records 50, 120 and 250, and a 10-base first exon in records 200 and 201."""
    rng = np.random.default_rng(23)
    g = acgt(rng, 300_000)
    recs = []
    for i in range(300):
        first = 10 if i in (200, 201) else 200
        recs.append([(0, 900 * i, first, False), (0, 900 * i + 250, 200, False),
                     (0, 900 * i + 500, 200, False)])
    for i in (50, 120, 250):
        g[900 * i + 300] = ord('S')
    return [g.tobytes()], tables(recs)


@pytest.mark.parametrize('lc', [3, 6])
def test_launch_order(slow_workload, monkeypatch, lc):
    monkeypatch.setenv('MAGOT_EXTRACT_LANE_CHUNKS', str(lc))
    monkeypatch.delenv('MAGOT_TILE_BLOCK_ROWS', raising=False)
    contigs, (ex, tx) = slow_workload
    plan = plan_debug(contigs, ex, tx)
    assert plan['lane_chunks'] == lc
    tiles, ex_g = plan['tiles'], [int(x) for x in plan['ex_g']]
    ex_out = plan['ex_out'].tolist()
    assert sum(bool(x & SLOWLIT) for x in ex_g) == 3
    slow = np.array([any(ex_g[e] & SLOWLIT or ex_out[e + 1] - ex_out[e] < CHUNK
                         for e in range(int(t['e1']), int(t['e2']))) for t in tiles])
    n_slow = int(slow.sum())
    assert 4 <= n_slow < len(tiles) // 2
    # tiles that may take the run-list path first, each group in output order
    assert slow[:n_slow].all() and not slow[n_slow:].any()
    T0 = tiles['T0'].astype(np.int64)
    assert (np.diff(T0[:n_slow]) > 0).all() and (np.diff(T0[n_slow:]) > 0).all()
    # and they are the cut's tiles
    in_order = tiles[np.argsort(T0)]
    assert np.array_equal(in_order, real_cut(ex_out, plan['tn'].tolist(), plan['tp'].tolist(), lc))
    assert np.array_equal(in_order, cut(ex_out, plan['tn'].tolist(), plan['tp'].tolist(), lc))


def test_tile_size_choice(slow_workload, monkeypatch):
    contigs, (ex, tx) = slow_workload
    monkeypatch.delenv('MAGOT_EXTRACT_LANE_CHUNKS', raising=False)
    monkeypatch.delenv('MAGOT_TILE_BLOCK_ROWS', raising=False)
    # far fewer large tiles than kSmallTilePlan: a translating plan gets the small tile
    both = plan_debug(contigs, ex, tx, _lib.OUT_NUC | _lib.OUT_PEP)
    assert both['lane_chunks'] == 3 and both['n_tiles'] < 40000
    assert plan_debug(contigs, ex, tx, _lib.OUT_PEP)['lane_chunks'] == 3
    nuc = plan_debug(contigs, ex, tx, _lib.OUT_NUC)
    assert nuc['lane_chunks'] == 6 and nuc['n_tiles'] < both['n_tiles']
    for force in (6, 3):
        monkeypatch.setenv('MAGOT_EXTRACT_LANE_CHUNKS', str(force))
        for outputs in (_lib.OUT_NUC | _lib.OUT_PEP, _lib.OUT_NUC):
            assert plan_debug(contigs, ex, tx, outputs)['lane_chunks'] == force


def test_block_rows_override(slow_workload, monkeypatch):
    contigs, (ex, tx) = slow_workload
    monkeypatch.setenv('MAGOT_TILE_BLOCK_ROWS', '%d,%d' % (BLK_EX, BLK_TX))
    plan = plan_debug(contigs, ex, tx)
    assert (plan['ex_rows'], plan['tx_rows'], plan['stride']) == (BLK_EX, BLK_TX, 768)
    monkeypatch.delenv('MAGOT_TILE_BLOCK_ROWS')
    plan = plan_debug(contigs, ex, tx)
    assert plan['ex_rows'] < BLK_EX and plan['stride'] == (32 + 8 * plan['ex_rows'] +
                                                           16 * plan['tx_rows'] + 15) & ~15


def test_unknown_output_flags(genome3):
    ex, tx = tables([[(0, 10, 30, False)]])
    with pytest.raises(_lib.MagotError) as err:
        plan_debug(genome3, ex, tx, 8)
    assert '(status -1): magot_plan_create: unknown output flags' in str(err.value)
