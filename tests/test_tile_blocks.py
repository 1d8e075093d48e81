"""Packed tile descriptor blocks (magot_amd/csrc/tileblocks.cpp).

CPU: the host packer, through magot_debug_tile_blocks, against the same
quantities computed from the u64 tables with Python integers.
GPU: extraction over plans whose tiles sit on the blocks' inline capacity,
byte for byte against cds_oracle, under both tile sizes.  A plan's blocks
hold what nearly all of its tiles stage (tile_geometry); the boundary cases
pin the capacity to the largest geometry, 64 interval rows and 14 record rows
(MAGOT_TILE_BLOCK_ROWS), and two cases run with the planner's own choice.

`cut` is an independent model of the planner's tile cut (binary searches
instead of cursors; tests/test_tileplan.py holds the planner to it).  The
workloads here are sized with the planner itself (`real_cut`, `plan_debug`),
so the GPU cases' "this workload stages m = ..." assertions speak about the
plan they run.
"""

from bisect import bisect_left, bisect_right
import ctypes

import numpy as np
import pytest

from magot_amd import _lib, synth

CHUNK, HALO = 16, 48
EXON_CAP, TX_CAP, PEP_SLOTS, TILE_ALIGN = 128, 64, 128, 128
BLK_EX, BLK_TX, NO_CHUNK = 64, 14, 511  # the largest block geometry (forced here)
RC, EXC, SLOWLIT = 1 << 63, 1 << 62, 1 << 61
M33 = (1 << 33) - 1
TILE_DTYPE = np.dtype([('T0', '<u8'), ('T1', '<u8'), ('Q0', '<u8'), ('Q1', '<u8'),
                       ('e1', '<u4'), ('e2', '<u4'), ('j1', '<u4'), ('j2', '<u4')])


def tile_bytes(lc):
    return (64 * lc - 3) * 16


def layout(rec_lens):
    """ex_out (n+1), tn / tp (codon-bearing records + sentinel) of records given
    as lists of non-empty interval lengths in output order."""
    ex_out, tn, tp = [0], [], []
    q = 0
    for lens in rec_lens:
        n = sum(lens)
        if n >= 3:
            tn.append(ex_out[-1])
            tp.append(q)
        for x in lens:
            ex_out.append(ex_out[-1] + x)
        q += n // 3
    tn.append(ex_out[-1])
    tp.append(q)
    return ex_out, tn, tp


def cut(ex_out, tn, tp, lc, T0=0, R0=0, max_tiles=1 << 30):
    """magot_plan_create's tiles from (T0, R0) on: rows of TILE_DTYPE."""
    Ec, Tc = len(ex_out) - 1, len(tn) - 1
    B, P, tile = ex_out[Ec], tp[Tc], tile_bytes(lc)

    def pcount(T):  # residues whose codon starts before T
        j = bisect_right(tn, T, 0, Tc)
        if j == 0:
            return 0
        return tp[j - 1] + min((T - tn[j - 1] + 2) // 3, tp[j] - tp[j - 1])

    def rec_of(q):
        return bisect_right(tp, q, 0, Tc) - 1

    out = []
    while T0 < B and len(out) < max_tiles:
        e1 = min(bisect_right(ex_out, T0) - 1, Ec)
        j1 = rec_of(R0) if R0 < P else Tc
        T1 = min(T0 + tile, B)
        if e1 + EXON_CAP < Ec:
            T1 = min(T1, ex_out[e1 + EXON_CAP] - HALO)
        if j1 + TX_CAP - CHUNK < Tc:
            T1 = min(T1, tn[j1 + TX_CAP - CHUNK])
        if T1 < B:
            T1 = T1 & ~(TILE_ALIGN - 1) if (T1 & ~(TILE_ALIGN - 1)) > T0 else T1 & ~(CHUNK - 1)
        if T1 < T0 + CHUNK:
            T1 = min(T0 + CHUNK, B)
        dec_end = min(T1 + HALO, B)
        R1 = P
        if T1 < B:
            R1 = min((pcount(T1) + CHUNK - 1) & ~(CHUNK - 1), P)
            R1 = min(R1, pcount(dec_end - 2))
            R1 = min(R1, (R0 & ~(CHUNK - 1)) + PEP_SLOTS * CHUNK)
        R1 = max(R1, R0)
        e2 = min(bisect_left(ex_out, dec_end), Ec)
        jl = rec_of(R1 - 1) if R1 > R0 else 0
        j2 = jl + 1 if R1 > R0 else j1
        assert e2 - e1 <= EXON_CAP and (R1 == R0 or j2 - j1 <= TX_CAP)
        out.append((T0, T1, R0, R1, e1, e2, j1 if R1 > R0 else 0, j2 if R1 > R0 else 0))
        T0, R0 = T1, R1
    return np.array(out, dtype=TILE_DTYPE)


def real_cut(ex_out, tn, tp, lc):
    """The planner's own cut of these tables (magot_debug_tile_cut), in output
    order: rows of TILE_DTYPE."""
    L = _lib.lib()
    a = [np.array(x, dtype=np.uint64) for x in (ex_out, tn, tp)]
    n = np.zeros(1, dtype=np.uint64)
    args = [_lib.ptr(a[0]), len(ex_out) - 1, _lib.ptr(a[1]), _lib.ptr(a[2]), len(tn) - 1, lc]
    _lib.check(L.magot_debug_tile_cut(*args, None, 0, _lib.ptr(n)), 'tile count')
    tiles = np.zeros(int(n[0]), dtype=TILE_DTYPE)
    _lib.check(L.magot_debug_tile_cut(*args, _lib.ptr(tiles), len(tiles), _lib.ptr(n)), 'tile cut')
    return tiles


PLAN_INFO = ('B', 'P', 'Ec', 'Tc', 'n_tiles', 'lane_chunks', 'ex_rows', 'tx_rows', 'stride')


def plan_debug(contigs, exons, txs, outputs=_lib.OUT_NUC | _lib.OUT_PEP):
    """What magot_plan_create plans for these contigs (bytes each) and tables,
    without a device (magot_debug_plan): a dict of PLAN_INFO integers and the
    tables ex_g, ex_out (Ec + 1), tn, tp (Tc + 1), lay_nuc, lay_pep (per
    record) and tiles (launch order).  Raises MagotError as plan creation would."""
    L = _lib.lib()
    bufs = [np.frombuffer(bytes(c), dtype=np.uint8) for c in contigs]
    ptrs = (ctypes.POINTER(ctypes.c_uint8) * max(len(bufs), 1))()
    for i, b in enumerate(bufs):
        if len(b):
            ptrs[i] = b.ctypes.data_as(ctypes.POINTER(ctypes.c_uint8))
    lens = np.array([len(b) for b in bufs], dtype=np.uint64)
    exons = np.ascontiguousarray(exons, dtype=_lib.EXON_DTYPE)
    txs = np.ascontiguousarray(txs, dtype=_lib.TX_DTYPE)
    info = np.zeros(len(PLAN_INFO), dtype=np.uint64)
    head = [ptrs, _lib.ptr(lens), len(bufs), _lib.ptr(exons), len(exons), _lib.ptr(txs), len(txs),
            outputs, _lib.ptr(info)]
    _lib.check(L.magot_debug_plan(*head, *[None] * 7), 'magot_debug_plan (sizes)')
    out = dict(zip(PLAN_INFO, (int(x) for x in info)))
    u8 = lambda n: np.zeros(n, dtype=np.uint64)
    out.update(ex_g=u8(out['Ec'] + 1), ex_out=u8(out['Ec'] + 1), tn=u8(out['Tc'] + 1),
               tp=u8(out['Tc'] + 1), lay_nuc=u8(len(txs)), lay_pep=u8(len(txs)),
               tiles=np.zeros(out['n_tiles'], dtype=TILE_DTYPE))
    _lib.check(L.magot_debug_plan(*head, *[_lib.ptr(out[k]) for k in (
        'ex_g', 'ex_out', 'tn', 'tp', 'lay_nuc', 'lay_pep', 'tiles')]), 'magot_debug_plan')
    return out


def find_length(make_lens, lc, want, lengths):
    """The first L of `lengths` for which the planner's cut of
    layout(make_lens(L)) has a tile with want(m, nt) true."""
    for L in lengths:
        t = real_cut(*layout(make_lens(L)), lc)
        m = t['e2'].astype(np.int64) - t['e1']
        nt = t['j2'].astype(np.int64) - t['j1']
        if any(want(int(a), int(b)) for a, b in zip(m, nt)):
            return L
    raise AssertionError('no length stages the wanted tile')


def const_exons(n_rec, n_ex):
    return lambda L: [[L] * n_ex for _ in range(n_rec)]


def single_exon(n_rec):
    return lambda L: [[L] for _ in range(n_rec)]


def full_exon_records():
    """Exons of 8-20 bases: tiles cut at kExonCap intervals.  (Uneven lengths:
    with a constant length the 128-byte rounding of the tile end always drops
    an interval or two.)"""
    rng = np.random.default_rng(0)
    return [[int(x) for x in rng.integers(8, 21, size=150)] for _ in range(40)]


# The most records the planner's cut can stage in one tile is kTxCap - 1: a tile
# ends at or before the start of record j1 + kTxCap - kChunk, and rounding its
# residues up to a 16-residue chunk adds at most kChunk - 1 one-residue records
# (with the sentinel row: kTxCap rows).  These single-exon records reach it in
# the plan's first tile: 48 records of 256 bytes and 81 residues, then
# one-residue records.
FULL_TX_RECORDS = [[4]] * 13 + [[3]] * 34 + [[102]] + [[3]] * 400


# ---------------------------------------------------------------------------
# CPU: the packer
# ---------------------------------------------------------------------------

def pack(ex_g, ex_out, tn, tp, span, lc, tiles, fill, rows):
    """(geometry [ex_rows, tx_rows, stride], blocks, overflow rows) for forced
    inline rows `rows` ((0, 0): the planner's choice)."""
    L = _lib.lib()
    a = [np.array(x, dtype=np.uint64) for x in (ex_g, ex_out, tn, tp)]
    n_ovf = np.zeros(2, dtype=np.uint64)
    geo = np.array([rows[0], rows[1], 0], dtype=np.uint32)
    args = [_lib.ptr(x) for x in a] + [span, lc, _lib.ptr(tiles), len(tiles), _lib.ptr(geo)]
    _lib.check(L.magot_debug_tile_blocks(*args, None, None, 0, None, 0, _lib.ptr(n_ovf)), 'sizes')
    ne, nx = int(n_ovf[0]), int(n_ovf[1])
    blocks = np.full(len(tiles) * int(geo[2]), fill, dtype=np.uint8)
    oex = np.full(max(ne, 1) * 8, fill, dtype=np.uint8)
    otx = np.full(max(nx, 1) * 16, fill, dtype=np.uint8)
    _lib.check(L.magot_debug_tile_blocks(*args, _lib.ptr(blocks), _lib.ptr(oex), ne, _lib.ptr(otx),
                                         nx, _lib.ptr(n_ovf)), 'pack')
    return [int(x) for x in geo], blocks, oex[:ne * 8], otx[:nx * 16]


def check_blocks(ex_g, ex_out, tn, tp, span, lc, tiles, rows=(BLK_EX, BLK_TX)):
    """Decode every block in numpy and compare each field with Python-integer
    arithmetic on the u64 tables.  Returns (set of m, set of nt, overflow rows,
    geometry)."""
    geo, blocks, oex, otx = pack(ex_g, ex_out, tn, tp, span, lc, tiles, 0x00, rows)
    geo2, b2, oex2, otx2 = pack(ex_g, ex_out, tn, tp, span, lc, tiles, 0xFF, rows)
    # every byte is written: the result does not depend on what was there
    assert geo == geo2
    assert np.array_equal(blocks, b2) and np.array_equal(oex, oex2) and np.array_equal(otx, otx2)
    E, X, stride = geo
    assert stride == (32 + 8 * E + 16 * X + 15) & ~15 and E % 2 == 0
    blk = blocks.reshape(len(tiles), stride)
    head64 = blk[:, :16].copy().view('<u8')
    head32 = blk[:, 16:32].copy().view('<u4')
    rows_ex = blk[:, 32:32 + 8 * E].copy().view('<u8')
    txr = blk[:, 32 + 8 * E:32 + 8 * E + 16 * X].copy().view('<i8').reshape(len(tiles), X, 2)
    assert not blk[:, 32 + 8 * E + 16 * X:].any()
    oex, otx = oex.view('<u8'), otx.view('<i8').reshape(-1, 2)
    end_cap = tile_bytes(lc) + 4 * HALO
    at_e = at_x = 0
    for t, tl in enumerate(tiles):
        T0, T1, Q0, Q1 = (int(tl[k]) for k in ('T0', 'T1', 'Q0', 'Q1'))
        e1, m = int(tl['e1']), int(tl['e2']) - int(tl['e1'])
        j1, nt = int(tl['j1']), int(tl['j2']) - int(tl['j1'])
        n_rows = nt + 1 if nt else 0
        assert m <= E + 64 and n_rows <= X + 64  # one overflow row per lane
        assert (int(head64[t, 0]), int(head64[t, 1])) == (T0, Q0)
        assert int(head32[t, 0]) == (T1 - T0) | (Q1 - Q0) << 16
        assert int(head32[t, 1]) == m | nt << 8
        assert int(head32[t, 2]) == (at_e if m > E else 0)
        assert int(head32[t, 3]) == (at_x if n_rows > X else 0)
        for j in range(max(E, m)):
            row = int(rows_ex[t, j]) if j < E else int(oex[at_e + j - E])
            if j >= m:
                assert row == 0  # padding a lane past m may load
                continue
            gw, o0, o1 = ex_g[e1 + j], ex_out[e1 + j], ex_out[e1 + j + 1]
            gs, s = gw & ~(RC | EXC | SLOWLIT), o0 - T0
            U = (2 * span - gs - (o1 - o0) - s) if gw & RC else gs - s
            lo, hi = row & 0xFFFFFFFF, row >> 32
            assert lo | (hi & 1) << 32 == U & M33, (t, j)
            assert (hi >> 1) & 0x1FFF == min(o1 - T0, end_cap)
            assert (hi >> 14) & 7 == bool(gw & RC) | bool(gw & EXC) << 1 | bool(gw & SLOWLIT) << 2
            assert (hi >> 17) & 0x1FF == (NO_CHUNK if j == 0 else min((s + 15) // 16, NO_CHUNK))
            assert hi >> 26 == 0
            if gw & RC:  # what the kernel derives for a reverse-forward row
                assert (2 * span - 16 - (U & M33)) & M33 == (gs + (o1 - T0) - 16) & M33
        for r in range(max(X, n_rows)):
            row = txr[t, r] if r < X else otx[at_x + r - X]
            want = (tn[j1 + r] - T0, tp[j1 + r] - Q0) if r < n_rows else (0, 0)
            assert (int(row[0]), int(row[1])) == want, (t, r)
        at_e += max(m - E, 0)
        at_x += max(n_rows - X, 0)
    assert at_e == len(oex) and at_x == len(otx)
    m = tiles['e2'].astype(np.int64) - tiles['e1']
    nt = tiles['j2'].astype(np.int64) - tiles['j1']
    return set(m.tolist()), set(nt.tolist()), (at_e, at_x), geo


def random_ex_g(rng, ex_out, span):
    """Interval words for a layout: random starts, strands and flag bits."""
    out = []
    for i in range(len(ex_out) - 1):
        n = ex_out[i + 1] - ex_out[i]
        gw = int(rng.integers(64, span - n - 64))
        gw |= RC if rng.random() < 0.5 else 0
        if rng.random() < 0.3:
            gw |= EXC | (SLOWLIT if not gw & RC and rng.random() < 0.5 else 0)
        out.append(gw)
    return out + [0]


@pytest.mark.parametrize('lc', [3, 6])
def test_packer_random_records(lc):
    rng = np.random.default_rng(7)
    recs = [[int(x) for x in rng.integers(1, 400, size=1 + rng.poisson(6))] for _ in range(600)]
    ex_out, tn, tp = layout(recs)
    span = 1 << 32
    tiles = cut(ex_out, tn, tp, lc)
    assert len(tiles) > 4 * 16
    ex_g = random_ex_g(rng, ex_out, span)
    check_blocks(ex_g, ex_out, tn, tp, span, lc, tiles)
    # the planner's own geometry: the rows of 98 % of the tiles are inline
    ms, nts, ovf, geo = check_blocks(ex_g, ex_out, tn, tp, span, lc, tiles, rows=(0, 0))
    m = np.sort(tiles['e2'].astype(np.int64) - tiles['e1'])
    nt = tiles['j2'].astype(np.int64) - tiles['j1']
    r = np.sort(np.where(nt > 0, nt + 1, 0))
    k = -(-len(tiles) * 49 // 50) - 1
    assert geo[0] == min((max(int(m[k]), 1, max(ms) - 64) + 1) & ~1, BLK_EX)
    assert geo[1] == min(max(int(r[k]), 1, int(r[-1]) - 64), BLK_TX)
    assert geo[0] < max(ms) and ovf[0] > 0


@pytest.mark.parametrize('lc', [3, 6])
def test_packer_interval_overflow_boundaries(lc):
    """Tiles of exactly kBlkEx (no overflow), kBlkEx + 1 (one overflow row) and
    kExonCap intervals."""
    rng = np.random.default_rng(8)
    span = 3 << 30
    for want_m in (BLK_EX, BLK_EX + 1, EXON_CAP):
        if want_m == EXON_CAP:
            ex_out, tn, tp = layout(full_exon_records())
        else:
            L = find_length(const_exons(40, 150), lc, lambda m, nt: m == want_m,
                            range(120, 8, -1))
            ex_out, tn, tp = layout(const_exons(40, 150)(L))
        ms, _, ovf, _ = check_blocks(random_ex_g(rng, ex_out, span), ex_out, tn, tp, span, lc,
                                  cut(ex_out, tn, tp, lc))
        assert want_m in ms
        assert (ovf[0] > 0) == (max(ms) > BLK_EX)


@pytest.mark.parametrize('lc', [3, 6])
def test_packer_record_overflow_boundaries(lc):
    """Tiles of kBlkTx - 1 records (kBlkTx rows with the sentinel: no overflow),
    kBlkTx (one overflow row), kTxCap - 1 (the most the planner cuts) and a
    hand-made tile of kTxCap records."""
    rng = np.random.default_rng(9)
    span = 1 << 31
    for want_nt in (BLK_TX - 1, BLK_TX, TX_CAP - 1):
        if want_nt == TX_CAP - 1:
            ex_out, tn, tp = layout(FULL_TX_RECORDS)
        else:
            L = find_length(single_exon(1500), lc, lambda m, nt: nt == want_nt,
                            range(600, 2, -3))
            ex_out, tn, tp = layout(single_exon(1500)(L))
        _, nts, ovf, _ = check_blocks(random_ex_g(rng, ex_out, span), ex_out, tn, tp, span, lc,
                                   cut(ex_out, tn, tp, lc))
        assert want_nt in nts
        assert (ovf[1] > 0) == (max(nts) + 1 > BLK_TX)
    ex_out, tn, tp = layout([[3]] * 200)
    tiles = np.array([(0, 192, 0, 64, 0, 80, 0, TX_CAP)], dtype=TILE_DTYPE)
    _, nts, ovf, _ = check_blocks(random_ex_g(rng, ex_out, span), ex_out, tn, tp, span, lc, tiles)
    assert nts == {TX_CAP} and ovf == (80 - BLK_EX, TX_CAP + 1 - BLK_TX)


@pytest.mark.parametrize('lc', [3, 6])
def test_packer_anchor_wraps_past_32_bits(lc):
    """A synthetic coordinate table (no genome): intervals that start more than
    2^32 bases before their tile's T0, on both strands, so U needs its bit 32;
    and intervals starting late in a tile at a small genome coordinate, so U
    wraps below 0."""
    big = (1 << 32) + 777
    recs = [[big, 40, 100], [90, big, 50], [300] * 5]
    ex_out, tn, tp = layout(recs)
    span = (1 << 32) + (1 << 12)
    # the long intervals at small / large starts, the short ones at coordinate 64
    # (gs - s < 0 for every tile they do not start)
    ex_g = [64, 64 | RC, 64, 64 | RC, 2000 | RC | EXC, 64 | EXC | SLOWLIT] + [64, 64 | RC] * 3
    ex_g = ex_g[:len(ex_out) - 1] + [0]
    # tiles over the end of each long interval and everything after it
    tiles = []
    for start in (big, ex_out[4] + big):
        T0 = (start - 3 * tile_bytes(lc)) & ~127
        Tc = len(tn) - 1
        j = bisect_right(tn, T0, 0, Tc)
        R0 = tp[j - 1] + min((T0 - tn[j - 1] + 2) // 3, tp[j] - tp[j - 1])
        tiles.append(cut(ex_out, tn, tp, lc, T0, (R0 + 15) & ~15, max_tiles=8))
    tiles = np.concatenate(tiles)
    assert any(int(t['T0']) - ex_out[int(t['e1'])] > 1 << 32 for t in tiles)
    check_blocks(ex_g, ex_out, tn, tp, span, lc, tiles)


def test_packer_rejects_bad_tiles():
    L = _lib.lib()
    ex_out, tn, tp = layout([[100] * 200])
    a = [np.array(x, dtype=np.uint64) for x in ([0] * 201, ex_out, tn, tp)]
    tiles = np.array([(0, 6016, 0, 2000, 0, 200, 0, 1)], dtype=TILE_DTYPE)  # 200 > kExonCap
    n_ovf = np.zeros(2, dtype=np.uint64)
    geo = np.zeros(3, dtype=np.uint32)
    rc = L.magot_debug_tile_blocks(*[_lib.ptr(x) for x in a], 1 << 20, 6, _lib.ptr(tiles), 1,
                                   _lib.ptr(geo), None, None, 0, None, 0, _lib.ptr(n_ovf))
    assert rc == _lib.ERR_RANGE


# ---------------------------------------------------------------------------
# GPU: plans on the capacity boundaries, against cds_oracle
# ---------------------------------------------------------------------------

@pytest.fixture(params=[3, 6])
def lane_chunks(request, monkeypatch):
    """Both tile sizes, blocks of the largest geometry (the capacity the
    boundary cases are built for)."""
    monkeypatch.setenv('MAGOT_EXTRACT_LANE_CHUNKS', str(request.param))
    monkeypatch.setenv('MAGOT_TILE_BLOCK_ROWS', '%d,%d' % (BLK_EX, BLK_TX))
    return request.param


@pytest.fixture(scope='module')
def base_workload():
    return synth.make('small', seed=11, genome_bases=1_000_000, n_tx=10, iupac_rate=1e-3)


def with_records(w, recs, genome=None):
    """A copy of workload w over records (contig, strand, start, [exon lengths
    ascending on the genome], intron)."""
    ex_start, ex_len = [], []
    for ctg, strand, start, lens, intron in recs:
        pos = start
        for n in lens:
            ex_start.append(pos)
            ex_len.append(n)
            pos += n + intron
        assert pos - intron <= int(w.contig_len[ctg]), 'record past its contig'
    i8 = np.int64
    return synth.Workload(w.name, w.genome if genome is None else genome, w.contig_len,
                          np.array([r[0] for r in recs], i8),
                          np.array([r[1] for r in recs], np.int8),
                          np.array([len(r[3]) for r in recs], i8), np.array(ex_start, i8),
                          np.array(ex_len, i8), w.outputs)


def staged(w, lc):
    """(m, nt) of every tile of the plan magot_plan_create builds for w (lc:
    the lane chunks the environment forces), and the tiles in output order."""
    ex, tx = w.plan_tables()
    plan = plan_debug([seq for _, seq in w.contigs()], ex, tx)
    assert plan['lane_chunks'] == lc
    t = plan['tiles'][np.argsort(plan['tiles']['T0'], kind='stable')]
    return list(zip((t['e2'].astype(np.int64) - t['e1']).tolist(),
                    (t['j2'].astype(np.int64) - t['j1']).tolist())), t


def trimmed(pep, poff):
    starts = poff[:-1].astype(np.int64)
    lens = (poff[1:] - poff[:-1]).astype(np.int64)
    first = np.zeros(len(starts), dtype=bool)
    nonempty = lens > 0
    first[nonempty] = pep[starts[nonempty]] == ord('X')
    keep = np.ones(len(pep), dtype=bool)
    keep[starts[first]] = False
    return pep[keep], lens - first


def check_against_oracle(w):
    from magot_amd import engine
    from oracle import cds_oracle
    dev = engine.DeviceGenome(w.contigs())
    ex, tx = w.plan_tables()
    plan = engine.ExtractionPlan(dev, ex, tx)
    nuc, noff, pep, poff = plan.run()
    plan.close()
    dev.close()
    ref, roff, st = cds_oracle.extract_workload(w, False)
    assert not st.any()
    assert np.array_equal(noff.astype(np.int64), roff)
    if not np.array_equal(nuc, ref):
        bad = int(np.nonzero(nuc != ref)[0][0])
        raise AssertionError('nucleotide mismatch at byte %d: %r vs %r' % (
            bad, nuc[max(0, bad - 8):bad + 8].tobytes(), ref[max(0, bad - 8):bad + 8].tobytes()))
    pref, proff, pst = cds_oracle.extract_workload(w, True)
    got, glen = trimmed(pep, poff)
    ok = pst == 0
    assert np.array_equal(glen[ok], (proff[1:] - proff[:-1])[ok])
    assert np.array_equal(got, pref)


def spread(w, n_rec, lens_of, intron=7):
    """n_rec records over the contigs, alternating strands (they may overlap on
    the genome: every record is extracted on its own)."""
    recs = []
    for i in range(n_rec):
        ctg = i % len(w.contig_len)
        lens = lens_of(i)
        room = int(w.contig_len[ctg]) - (sum(lens) + intron * len(lens)) - 1
        recs.append((ctg, 1 if i % 2 == 0 else -1, (i * 7919) % room, lens, intron))
    return recs


@pytest.mark.gpu
@pytest.mark.parametrize('which', ['cap', 'cap+1', 'full'])
def test_gpu_interval_capacity_boundary(base_workload, lane_chunks, which):
    """Constant exon lengths chosen so that tiles stage exactly kBlkEx and
    kBlkEx + 1 intervals, and 8-20 base exons for kExonCap."""
    want_m = {'cap': BLK_EX, 'cap+1': BLK_EX + 1, 'full': EXON_CAP}[which]
    if which == 'full':
        lens = full_exon_records()
    else:
        L = find_length(const_exons(40, 150), lane_chunks, lambda m, nt: m == want_m,
                        range(120, 8, -1))
        lens = const_exons(40, 150)(L)
    w = with_records(base_workload, spread(base_workload, 40, lambda i: lens[i]))
    assert any(m == want_m for m, _ in staged(w, lane_chunks)[0])
    check_against_oracle(w)


@pytest.mark.gpu
@pytest.mark.parametrize('which', ['cap', 'cap+1', 'full'])
def test_gpu_record_capacity_boundary(base_workload, lane_chunks, which):
    """Single-exon records sized so that tiles hold kBlkTx - 1 records (with the
    sentinel: exactly the inline rows), kBlkTx (one overflow row) and kTxCap - 1
    (kTxCap rows: the most the planner's cut stages, FULL_TX_RECORDS)."""
    want_nt = {'cap': BLK_TX - 1, 'cap+1': BLK_TX, 'full': TX_CAP - 1}[which]
    if which == 'full':
        lens = FULL_TX_RECORDS
    else:
        L = find_length(single_exon(1500), lane_chunks, lambda m, nt: nt == want_nt,
                        range(600, 2, -3))
        lens = single_exon(1500)(L)
    w = with_records(base_workload, spread(base_workload, len(lens), lambda i: lens[i]))
    assert any(nt == want_nt for _, nt in staged(w, lane_chunks)[0])
    check_against_oracle(w)


@pytest.mark.gpu
def test_gpu_both_overflows(base_workload, lane_chunks):
    """Records of four 12-base exons: a tile overflows its interval rows and its
    record rows at once."""
    w = with_records(base_workload, spread(base_workload, 900, lambda i: [12] * 4))
    assert any(m > BLK_EX and nt + 1 > BLK_TX for m, nt in staged(w, lane_chunks)[0])
    check_against_oracle(w)


@pytest.mark.gpu
def test_gpu_long_intervals(base_workload, lane_chunks):
    """Intervals several tiles long on both strands, clean (a '-' one is a
    reverse-forward row) and over an exception byte (mirror rows, one needing
    the run list): the first, middle and last tiles of an interval see the same
    row at very different tile-relative starts."""
    w0 = base_workload
    g = w0.genome.copy()
    n = 20_011
    ctgs = np.argsort(-w0.contig_len)[:2]
    recs = []
    for k, (exc, strand) in enumerate([(None, 1), (None, -1), (b'N', 1), (b'N', -1), (b'S', 1),
                                       (b'S', -1)]):
        ctg = int(ctgs[k % 2])
        start = 1000 + (k // 2) * (n + 500)
        a = int(w0.contig_off[ctg]) + start
        seg = g[a:a + n + 300]
        seg[~np.isin(seg, np.frombuffer(b'ACGTacgt', np.uint8))] = ord('A')
        if exc:
            seg[n // 2] = exc[0]
        # a second, short interval so that the long one is not the whole record
        recs.append((ctg, strand, start, [n, 200], 100))
    w = with_records(w0, recs, genome=g)
    assert int(w.contig_len[ctgs[1]]) > 3 * (n + 500) + 2000
    check_against_oracle(w)


@pytest.mark.gpu
@pytest.mark.parametrize('which', ['one_tile', 'short_last_tile'])
def test_gpu_short_plans(base_workload, lane_chunks, which):
    """A plan of one tile; a plan whose last tile is shorter than a chunk."""
    ctg = int(np.argmax(base_workload.contig_len))
    if which == 'one_tile':
        recs = [(ctg, -1, 500, [300], 0)]
    else:
        # 48 records of 256 bytes in all, then one of 7 bases: the first tile
        # ends at the start of record 48 (a tile holds whole records up to
        # j1 + kTxCap - kChunk), on a 128-byte line
        lens = FULL_TX_RECORDS[:48] + [[7]]
        recs = spread(base_workload, len(lens), lambda i: lens[i])
    w = with_records(base_workload, recs)
    tiles = staged(w, lane_chunks)[1]
    if which == 'one_tile':
        assert len(tiles) == 1
    else:
        assert int(tiles[-1]['T1']) - int(tiles[-1]['T0']) == 7
    check_against_oracle(w)


@pytest.mark.gpu
def test_gpu_planner_geometry(base_workload, lane_chunks, monkeypatch):
    """The planner's own block geometry: most records have 200-base exons, a
    few 40-base ones, so the blocks hold the common tiles' rows and the few
    tiles over the short exons overflow; and the short-record plan, whose
    record rows overflow."""
    monkeypatch.delenv('MAGOT_TILE_BLOCK_ROWS')
    lens = [[200] * 60] * 60 + [[40] * 150] * 2
    w = with_records(base_workload, spread(base_workload, len(lens), lambda i: lens[i]))
    m = sorted(a for a, _ in staged(w, lane_chunks)[0])
    assert m[-1] > m[len(m) * 49 // 50] + 2  # some tiles stage more than the inline rows
    check_against_oracle(w)
    lens = [[300]] * 600 + FULL_TX_RECORDS
    w = with_records(base_workload, spread(base_workload, len(lens), lambda i: lens[i]))
    check_against_oracle(w)
