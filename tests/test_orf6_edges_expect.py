"""The builders of orf6_expect.py hold what they are named for, the model's
tiles are the planner's own (magot_debug_orf6_tiles: this also pins the tile
size and the row cap that test_orf6_plan.py writes down), and the expected
bytes are the oracle's translate().  No device: this is what keeps a test of
test_gpu_orf6_edges.py from passing beside its point."""

import os

import numpy as np
import pytest

import orf6_expect as oe
from magot_amd import _lib, engine
from oracle import magot_oracle as mo
from test_orf6_plan import orf6_windows
from test_tile_blocks import plan_debug

TILE = oe.TILE


def _same_tiles(model, planner):
    keys = [k for k in ('T0', 'T1', 'r0', 'e0', 'm') if k in planner[0]] if planner else []
    assert [[t[k] for k in keys] for t in model] == [[t[k] for k in keys] for t in planner]
    for t in model:
        assert t['W0'] == (max(t['T0'] - 48, 0) & ~15) and t['WE'] - t['T1'] in range(51)


def _raw(records):
    """The model of a raw-mode input, held to the planner and to the ownership
    invariants."""
    noff = oe.offsets(len(r) for r in records)
    tiles = oe.decompose(noff)
    _same_tiles(tiles, oe.planner_tiles(noff))
    oe.check_partition(noff, tiles)
    return noff, tiles


def _fused(w, order):
    d = plan_debug([w.genome.tobytes()], w.ex, w.tx, _lib.OUT_NUC)
    perm, noff, starts, rows = w.walk(d['ex_g'], order)
    assert noff[-1] == d['B'] and len(rows) == d['Ec']
    tiles = oe.decompose(noff, starts)
    _same_tiles(tiles, oe.planner_tiles(noff, starts))
    oe.check_partition(noff, tiles)
    return perm, noff, starts, rows, tiles


def _chunks(tiles):
    for t in tiles:
        for b in t['batches']:
            for c in b['chunks']:
                yield t, b, c


def test_the_constants_are_the_planner_s():
    """A record of two tiles and a base is cut at the tile size; 124 one-base
    intervals are cut at the row cap."""
    assert [t['T1'] for t in oe.planner_tiles([0, 2 * TILE + 1])] == [TILE, 2 * TILE, 2 * TILE + 1]
    assert (oe.TILE, oe.CAP) == (3968, 123)
    starts = list(range(oe.CAP + 2))
    t = oe.planner_tiles([0, oe.CAP + 1], starts)
    assert t[0]['T1'] == oe.CAP - 50 and t[0]['m'] == oe.CAP
    assert oe.planner_tiles([0], None) == [] and oe.planner_tiles([0, 0, 0], [0]) == []


# ---------------------------------------------------------------------------
# (a)
# ---------------------------------------------------------------------------

def test_lengths_hold_every_residue_class_and_none_stream():
    recs = oe.lengths_all()
    assert [len(r) for r in recs] == list(range(201))
    noff, tiles = _raw(recs)
    soff, slen = oe.sizes([len(r) for r in recs])
    assert {(j % 6, n % 16) for j, n in enumerate(slen)} == \
        {(k, q) for k in range(6) for q in range(16)}
    none = {(L, f) for L in range(9) for f in range(3) if mo.translate('A' * L, frame=f) is None}
    assert none == {(L, f) for L in range(9) for f in range(3) if L <= 2 + f}
    # the last chunk of a stream leaves every count 1..16 on both strands
    assert {(c[0], min(c[6], 16)) for _, _, c in _chunks(tiles)} == \
        {(s, n) for s in (True, False) for n in range(1, 17)}


def test_a_short_first_record_reads_the_guards():
    seen = set()
    for L in oe.FIRST_LENGTHS:
        recs = oe.lengths_first(L)
        assert len(recs[0]) == L
        noff, tiles = _raw(recs)
        assert tiles[0]['W0'] == 0
        seen |= {c[5] for _, _, c in _chunks(tiles) if not c[0] and c[1] == 0}
    assert seen >= set(range(-45, 0)) and min(seen) == -45   # P of '-' chunks of record 0


def test_record_counts_in_one_tile():
    for n in oe.N_RECS:
        recs = oe.lengths_n_rec(n)
        noff, tiles = _raw(recs)
        assert len(recs) == n and len(tiles) == 1
        assert len(tiles[0]['batches']) == (n + oe.BATCH - 1) // oe.BATCH
        assert tiles[0]['batches'][-1]['rb'] + oe.BATCH >= n


# ---------------------------------------------------------------------------
# (b)
# ---------------------------------------------------------------------------

def test_seams_hold_every_phase_of_both_ownership_formulas():
    recs = oe.seams()
    noff, tiles = _raw(recs)
    phases, near = oe.seam_cases(noff, tiles)
    assert phases == {(s, f, p) for s in (True, False) for f in range(3) for p in range(48)}
    assert near == {(s, f, d) for s in (True, False) for f in range(3) for d in (-1, 0, 1)}
    seams = {t['T0'] for t in tiles[1:]}
    assert {e - T for e in noff[1:] for T in seams if abs(e - T) <= 1} == {-1, 0, 1}
    assert tiles[0]['W0'] == 0 and tiles[0]['T0'] == 0
    assert tiles[-1]['WE'] == noff[-1] and tiles[-1]['T1'] == noff[-1]
    assert all(t['WE'] == t['T1'] + 50 for t in tiles[:-2])
    assert max(len(r) for r in recs) > 3 * TILE
    assert noff[-1] < 1 << 20


# ---------------------------------------------------------------------------
# (c)
# ---------------------------------------------------------------------------

def test_batches_hold_their_record_counts_and_the_tenth_record_s_end():
    recs = oe.batches()
    noff, tiles = _raw(recs)
    assert all(t['T1'] - t['T0'] == TILE for t in tiles)
    touch = [oe.touching(noff, t) for t in tiles]
    assert touch[:len(oe.TOUCHING)] == list(oe.TOUCHING)
    # the run of empty records: batches that own nothing and go on by `more`
    t = tiles[len(oe.TOUCHING)]
    idle = [b for b in t['batches'] if b['n_chunks'] == 0]
    assert len(t['batches']) == 101 and len(idle) == 99 and all(b['more'] for b in idle)
    assert t['batches'][-1]['n_chunks'] > 0
    # the tenth record of a tile's first batch against T1
    seen = {}
    for t in tiles:
        b = t['batches'][0]
        end = noff[b['rb'] + oe.BATCH] if b['rb'] + oe.BATCH < len(noff) else None
        if end is not None and abs(end - t['T1']) <= 1 and noff[b['rb']] == t['T0']:
            seen[end - t['T1']] = (b['more'], len(t['batches']))
    assert seen == {-1: (True, 2), 0: (False, 1), 1: (False, 1)}


# ---------------------------------------------------------------------------
# (d)
# ---------------------------------------------------------------------------

def test_chunk_passes_hold_their_counts_and_variants():
    modes = {}
    for n in oe.PER_STRAND:
        recs = oe.chunk_counts(n)
        noff, tiles = _raw(recs)
        assert len(tiles) == 1 and len(tiles[0]['batches']) == 1
        b = tiles[0]['batches'][0]
        assert (b['n_minus'], b['n_chunks'] - b['n_minus']) == (n, n)
        modes[n] = oe.modes_of(b)
    assert modes == {1: [2], 63: [2, 0], 64: [1, 0], 65: [1, 2, 0], 128: [1, 1, 0, 0]}


def test_segment_starts_fall_on_every_bit_of_three_words():
    noff, tiles = _raw(oe.segment_bits())
    seen, words = set(), set()
    for t in tiles:
        for b in t['batches']:
            seen |= {(min(s >> 5, 2), s & 31) for s in b['seg_start']}
            words |= {s >> 5 for s in b['seg_start']}
    assert seen == {(w, bit) for w in range(3) for bit in range(32)}
    assert max(words) >= 4


# ---------------------------------------------------------------------------
# (e)
# ---------------------------------------------------------------------------

def test_invalid_bytes_fall_on_every_window_position_and_shift():
    seen, met = set(), set()
    for part in range(oe.INVALID_PARTS):
        recs = oe.invalid(part)
        noff, tiles = _raw(recs)
        assert noff[-1] < 1 << 20
        got, dirty, b = oe.invalid_cases(recs, tiles)
        seen |= got
        met |= b
        pairs = set(zip(dirty, dirty[1:]))
        assert {(True, False), (False, True), (False, False)} <= pairs
    assert seen == {(s, j, p) for s in (True, False) for j in range(48) for p in range(32)}
    assert met == set(oe.BAD_BYTES)


# ---------------------------------------------------------------------------
# (f), (g)
# ---------------------------------------------------------------------------

@pytest.mark.parametrize('order', oe.ORDERS)
def test_fused_pairs_hold_every_join(order):
    w = oe.fused_pairs()
    perm, noff, starts, rows, tiles = _fused(w, order)
    c = oe.fused_cases(tiles, starts, rows)
    sides = {(s, a) for s in (False, True) for a in range(16)}
    assert c['pair'] == {(j0, s0, s1, f0, f1) for j0 in range(1, 16) for s0 in (False, True)
                         for s1 in (False, True) for f0 in (False, True) for f1 in (False, True)}
    assert c['a0'] == sides and c['a1'] == sides
    assert c['shift0'] == set(range(32)) and c['shift1'] == set(range(32))
    assert c['spans'] == {1, 2}
    # (g): empty records last in genome order, equal keys in record order
    empty = [r for r in range(len(w.records)) if noff_len(w, r) == 0]
    assert len(empty) >= 20
    twins = [r for r in range(1, len(w.records))
             if w.records[r] and w.records[r] == w.records[r - 1]]
    assert len(twins) >= 10
    if order == 'genome':
        assert perm != sorted(perm) and perm[-len(empty):] == empty
        assert all(perm.index(r) == perm.index(r - 1) + 1 for r in twins)
    else:
        assert perm == sorted(perm)


def noff_len(w, r):
    return sum(ln for _, ln, _ in w.records[r])


@pytest.mark.parametrize('order', oe.ORDERS)
def test_fused_exact_vectors_hold_every_nibble_shift(order):
    w = oe.fused_exact()
    perm, noff, starts, rows, tiles = _fused(w, order)
    c = oe.fused_cases(tiles, starts, rows)
    assert c['exact'] >= {(k, a, h) for k in oe.EXACT_SPANS for a in range(8) for h in (0, 1)}
    assert c['spans'] >= {1} | set(oe.EXACT_SPANS)
    flagged = {f for _, f, _ in rows}
    assert flagged == {False, True} and {s for _, _, s in rows} == {False, True}


@pytest.mark.parametrize('order', oe.ORDERS)
def test_fused_windows_stage_every_row_count(order):
    for m in oe.ROWS_STAGED:
        perm, noff, starts, rows, tiles = _fused(oe.fused_rows(m), order)
        assert len(tiles) == 1 and tiles[0]['m'] == m and 'capped' not in tiles[0]
    for k in oe.ONLY_FLAGGED:
        w = oe.fused_rows(oe.CAP, flagged=k)
        perm, noff, starts, rows, tiles = _fused(w, order)
        assert len(tiles) == 1 and oe.fused_cases(tiles, starts, rows)['only_flag'] == {k}
    assert min(oe.ONLY_FLAGGED) == 64 and max(oe.ONLY_FLAGGED) == oe.CAP - 1


@pytest.mark.parametrize('order', oe.ORDERS)
def test_fused_row_cap_shortens_the_tiles(order):
    w = oe.fused_cap()
    perm, noff, starts, rows, tiles = _fused(w, order)
    c = oe.fused_cases(tiles, starts, rows)
    assert c['capped'] == {'cap-50'} and oe.CAP in c['m'] and 16 in c['spans']
    short = [t for t in tiles[:-1] if t['T1'] - t['T0'] < TILE]
    assert len(short) >= 10 and all('capped' in t for t in short)
    one = [r for r in rows if r[2]]                      # alternating strands
    assert len(one) >= 200 and len(rows) - len(one) >= 200


@pytest.mark.parametrize('order', oe.ORDERS)
def test_fused_edges_hold_long_rows_and_the_contig_s_ends(order):
    w = oe.fused_edges()
    perm, noff, starts, rows, tiles = _fused(w, order)
    c = oe.fused_cases(tiles, starts, rows)
    assert c['before_w0'] and len(tiles) >= 6
    d = plan_debug([w.genome.tobytes()], w.ex, w.tx, _lib.OUT_NUC)
    u = [int(g) & ((1 << 61) - 1) for g in d['ex_g'][:-1]]
    first = min(u)
    lens = w.ex['len'][w.ex['len'] > 0]
    assert u.count(first) >= 3
    assert max(x + int(ln) for x, ln in zip(u, lens)) == first + oe.G_LEN


@pytest.mark.parametrize('order', oe.ORDERS)
@pytest.mark.parametrize('name', sorted(oe.RAW_OVER_PLAN))
def test_raw_builders_over_a_plan_keep_their_records(name, order):
    """(a)-(c) through the fused path: one interval per record, alternating
    strands; the gathered records are the raw ones, the tiles the planner's."""
    recs = oe.RAW_OVER_PLAN[name]()
    w = oe.over_genome(recs)
    assert all(np.array_equal(a, b) for a, b in zip(w.record_bytes(), recs))
    perm, noff, starts, rows, tiles = _fused(w, order)
    assert {s for _, _, s in rows} == {False, True} and not any(f for _, f, _ in rows)
    if name == 'batches':       # 400 rows in a tile: cut at the row cap, ten batches in one
        assert any('capped' in t for t in tiles) and max(len(t['batches']) for t in tiles) >= 10
    elif order == 'record':
        raw = oe.tiles_of(oe.offsets(len(r) for r in recs))
        cut = lambda ts: [(t['T0'], t['T1'], t['r0']) for t in ts]
        assert cut(raw) == cut(tiles)


@pytest.mark.parametrize('name', sorted(oe.FUSED))
def test_the_model_s_windows_are_orf6_windows(name):
    """Record order: rows, row counts and flagged rows of every window as
    test_orf6_plan.orf6_windows restates them from the genome's bytes."""
    w = oe.FUSED[name]()
    perm, noff, starts, rows, tiles = _fused(w, 'record')
    wins = orf6_windows(w)
    assert [(t['e0'], t['m']) for t in tiles] == [(e, min(m, oe.CAP)) for e, m, _ in wins]
    for t, (e, m, flagged) in zip(tiles, wins):
        mine = [i for i in range(t['m']) if rows[e + i][1]]
        assert mine == [i for i in flagged.tolist() if i < t['m']]


# ---------------------------------------------------------------------------
# the expected bytes
# ---------------------------------------------------------------------------

def _golden_records():
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden',
                        'O.biroi_refseqGenomeSubset.fasta')
    seqs, cur = [], []
    with open(path) as fh:
        for line in fh:
            if line.startswith('>'):
                if cur:
                    seqs.append(''.join(cur))
                cur = []
            else:
                cur.append(line.strip())
    seqs.append(''.join(cur))
    out = []
    for i, s in enumerate(seqs):
        out += [s[:1000 + i], s[5000:5000 + 997 + 3 * i], s[-(700 + i):]]
    return out


FIXED = ['', 'A', 'AC', 'ACG', 'ACGT', 'ACGTA', 'ACGTAC', 'ACGTACG', 'ACGTACGT',
         'ATGGCCTTTAAACCCGGGTAG', 'atgNNNcctRYKMSWtag-*-ACGTnnacgtTGA', 'Nn-RYKMS*' * 7,
         'TTTTCTTATTGTTAATAGTGActgccccatcaacgg' * 5 + 'AT', '\xe9\xdfACGT\xb5\x00ACGTT']


def test_expected_streams_are_the_oracle_s_translate():
    w = oe.fused_edges()
    recs = FIXED + _golden_records() + \
        [r.tobytes().decode('latin-1') for r in w.record_bytes() if len(r) < 2000]
    arrs = [np.frombuffer(s.encode('latin-1'), np.uint8) for s in recs]
    buf, soff, slen = oe.expected(arrs)
    for r, s in enumerate(recs):
        for f in range(3):
            for st in (0, 1):
                t = mo.translate(s, frame=f, strand='-+'[st], trimX=False)
                want = '' if t is None else t[1:] if f else t
                j = 6 * r + 2 * f + st
                assert oe.orf_count(len(s), f) == len(want) == int(slen[j])
                got = oe.stream(arrs[r], f, st == 0)
                assert got.tobytes().decode('latin-1') == want, (r, f, st)
                assert np.array_equal(buf[int(soff[j]):int(soff[j]) + len(want)], got)
    # the layout: magot_orf6_sizes' table, and nothing but zeros between streams
    ref_soff, ref_slen = engine.orf6_sizes(np.array(oe.offsets(len(s) for s in recs)))
    assert np.array_equal(soff, ref_soff) and np.array_equal(slen, ref_slen)
    assert int((buf != 0).sum()) == int(slen.sum())


def test_the_fused_records_are_the_oracle_s_gather():
    """Fused.record_bytes: intervals cut from the contig and reverse-
    complemented by the oracle, '-' records of the contig's ends included."""
    w = oe.fused_edges()
    text = w.genome.tobytes().decode('latin-1')
    got = w.record_bytes()
    assert got[0].tobytes().decode('latin-1') == text[:40]
    assert got[3].tobytes().decode('latin-1') == mo.reverse_complement(text[-33:])
    assert [len(r) for r in got] == [noff_len(w, r) for r in range(len(w.records))]


def test_first_difference_names_the_stream():
    recs = oe.raw_case([40, 100], 9)
    buf, soff, slen = oe.expected(recs)
    assert oe.first_difference(buf, buf, soff, slen) is None
    bad = buf.copy()
    at = int(soff[6 + 2 * 1 + 1]) + 5            # record 1, frame 1, '+', residue 5
    bad[at] ^= 1
    msg = oe.first_difference(bad, buf, soff, slen)
    assert msg.startswith('byte %d:' % at) and 'record 1, frame 1, strand +, residue 5' in msg
