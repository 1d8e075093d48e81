"""orf6_kernel (magot_amd/csrc/seqops.hip) at its own edges: a CPU model of how
the kernel cuts its work, deterministic inputs built for each cut, and the
bytes the kernel must write for them (test infrastructure).

The model restates, with Python integers, orf6_plan_tiles (tiles and their
staged windows), the fused staging's per-vector interval lookup, the record
batches of 10 with their lanes' chunk ownership (lo, hi), the chunk bitmap's
segment starts, and every chunk's strand, window position P and residues left.
It extends tests/test_orf6_plan.py (whose tile size and row cap it uses, and
whose orf6_windows it is held against).  What the model says of a builder is
asserted in test_orf6_edges_expect.py, where the tiles are also compared with
the planner's own (magot_debug_orf6_tiles); test_gpu_orf6_edges.py runs the
builders on the device.

  (a) lengths  every record length 0..200 (every residue of nres mod 16 in all
               six streams, None streams by frame), a first record of 3..47
               bases ('-' chunks at P < 0: the guards), 1..11, 20, 21 records
               in one tile
  (b) seams    a record over a tile seam at every phase mod 48, per frame and
               strand (288 cases), chunks whose first codon starts at T1-1,
               T1, T1+1, record ends at T0-1, T0, T0+1, the first and the last
               tile, a record longer than three tiles
  (c) batches  tiles touching 1, 9, 10, 11, 20, 21 and 400 records, 1,000
               empty records in a row, the batch's tenth record ending at
               T1-1, T1, T1+1
  (d) chunks   1, 63, 64, 65, 128 chunks per strand in a batch, the three
               chunk variants in one batch, segment starts on every bit of a
               bitmap word in words 0, 1 and beyond
  (e) invalid  one non-ACGT byte at every position of a chunk's 48-base window
               for every P & 31 on both strands, each of N n - R Y K M S *,
               clean tiles beside dirty ones
  (f) fused    vectors over two intervals (j0 = 1..15, every A & 15 on each
               side, the strand pairs, the flag pairs, every exception-plane
               shift), over 3, 4 and 16 intervals (the exact path), windows of
               1..123 rows, the row cap, an only flagged row at 64..122,
               intervals from before W0, the plane's first and last base
  (g) order    the fused builders in record order and in genome order, with
               empty records and records of equal keys among them

Not reachable at this size: a row more than 2^30 bases before its window (the
clamp of rel), and planes of 4 GiB (the buffer range clamp).  Not reachable at
any size: the T + 1 arm of the row cap's max(T + 1, cap - 50): row e holds W0
> T - 64 and non-empty intervals are at least one base, so cap >= T + 60; and
a wrong answer from reading `more` off lane 57 or 58, which hold the same
record as lane 59."""

import ctypes

import numpy as np

from magot_amd import _lib
from oracle import magot_oracle as mo
from test_orf6_plan import ORF_TILE, ROW_CAP

TILE, CAP = ORF_TILE, ROW_CAP
BATCH, SEGS = 10, 60
RC = 1 << 63
EXC = 1 << 62
ACGT = np.frombuffer(b'ACGTacgt', dtype=np.uint8)
BAD_BYTES = b'Nn-RYKMS*'


# ---------------------------------------------------------------------------
# expected bytes, from the oracle's tables (checked against its translate())
# ---------------------------------------------------------------------------

def _classes():
    cls = {'+': np.full(256, 4, np.int64), '-': np.full(256, 4, np.int64)}
    for b in range(256):
        ch = chr(b)
        for strand, x in (('+', ch), ('-', mo._RC_MAP.get(ch, 'n'))):
            u = x.upper()
            if len(u) == 1 and u in 'ACGT':
                cls[strand][b] = 'ACGT'.index(u)
    lut = np.zeros(125, np.uint8)
    for i in range(125):
        trip = ''.join('ACGTN'[(i // d) % 5] for d in (25, 5, 1))
        lut[i] = ord(mo.STANDARD_CODE.get(trip, 'X'))
    return cls, lut


_CLS, _LUT = _classes()


def orf_count(L, f):
    """Real codons of frame f in a record of L bases (0 where translate() is
    None or has only its junk residue)."""
    return (L - 2 * f) // 3 if (L > 2 + f and L >= 2 * f + 3) else 0


def stream(rec, f, minus):
    """The residues of one stream of a record (uint8 array): translate(frame=f,
    strand, trimX=False) without the junk first residue of frames 1 and 2."""
    n = orf_count(len(rec), f)
    if n == 0:
        return np.zeros(0, np.uint8)
    c = _CLS['-'][rec[::-1]] if minus else _CLS['+'][rec]
    c = c[2 * f:2 * f + 3 * n].reshape(n, 3)
    return _LUT[c[:, 0] * 25 + c[:, 1] * 5 + c[:, 2]]


def sizes(lens, order=None):
    """magot_orf6_sizes restated, with the records' blocks laid out in walk
    order: (soff 6n+1, slen 6n), stream j = 6 r + 2 f + (strand == '+')."""
    n = len(lens)
    order = range(n) if order is None else order
    soff, slen = [0] * (6 * n + 1), [0] * (6 * n)
    acc = 0
    for r in order:
        for st in (0, 1):
            for f in range(3):
                j = 6 * r + 2 * f + st
                slen[j] = orf_count(lens[r], f)
                soff[j] = acc
                acc += (slen[j] + 15) & ~15
    soff[6 * n] = acc
    return soff, slen


def expected(records, order=None):
    """(buffer, soff, slen): every stream at its place, zeros up to the next
    16-byte boundary, nothing else."""
    soff, slen = sizes([len(r) for r in records], order)
    buf = np.zeros(soff[-1], np.uint8)
    for r, rec in enumerate(records):
        for st in (0, 1):
            for f in range(3):
                j = 6 * r + 2 * f + st
                if slen[j]:
                    buf[soff[j]:soff[j] + slen[j]] = stream(rec, f, st == 0)
    return buf, np.array(soff, np.uint64), np.array(slen, np.uint64)


def first_difference(got, want, soff, slen):
    """None, or a description of the first differing byte: its offset, and the
    record, stream and residue whose padded place holds it."""
    if len(got) != len(want):
        return 'length %d, expected %d' % (len(got), len(want))
    bad = np.nonzero(got != want)[0]
    if not len(bad):
        return None
    at = int(bad[0])
    start = np.asarray(soff[:-1], np.int64)
    end = start + ((np.asarray(slen, np.int64) + 15) & ~15)
    j = int(np.nonzero((start <= at) & (at < end))[0][0])
    return ('byte %d: got 0x%02x, expected 0x%02x; record %d, frame %d, strand %s, '
            'residue %d of %d (%d bytes differ)' % (at, got[at], want[at], j // 6, (j % 6) // 2, '-+'[j % 2],
                                   at - int(soff[j]), int(slen[j]), len(bad)))


def bases(n, seed):
    return ACGT[np.random.default_rng(seed).integers(0, 8, size=n)]


def cut(buf, lens):
    off = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    return [buf[off[i]:off[i + 1]] for i in range(len(lens))]


# ---------------------------------------------------------------------------
# the model
# ---------------------------------------------------------------------------

def offsets(lens):
    out = [0]
    for L in lens:
        out.append(out[-1] + int(L))
    return out


def tiles_of(noff, starts=None):
    """orf6_plan_tiles: per tile T0, T1, W0, WE, r0 and, over interval rows
    (`starts`: the non-empty intervals' starts, then the total), e0 and m."""
    n_rec = len(noff) - 1
    total = noff[n_rec] if n_rec else 0
    n_rows = len(starts) - 1 if starts is not None else 0
    out = []
    r = e = f = 0
    T = 0
    while T < total:
        W0 = (T - 48 if T >= 48 else 0) & ~15
        while r + 1 < n_rec and noff[r + 1] <= T:
            r += 1
        T1 = min(T + TILE, total)
        t = dict(T0=T, r0=r, W0=W0)
        if starts is not None:
            while e + 1 < n_rows and starts[e + 1] <= W0:
                e += 1
            if e + CAP < n_rows:
                cap = starts[e + CAP]
                if T1 + 50 > cap:
                    T1 = max(T + 1, cap - 50)
                    t['capped'] = 'T+1' if T + 1 > cap - 50 else 'cap-50'
            WE = min(T1 + 50, total)
            f = max(f, e)
            while f < n_rows and starts[f] < WE:
                f += 1
            t.update(e0=e, m=min(f - e, CAP))
        t.update(T1=T1, WE=min(T1 + 50, total))
        out.append(t)
        T = T1
    return out


def planner_tiles(noff, starts=None):
    """The same from the planner itself (magot_debug_orf6_tiles)."""
    L = _lib.lib()
    a = np.array(noff, dtype=np.uint64)
    s = None if starts is None else np.array(starts, dtype=np.uint64)
    n = ctypes.c_uint64()
    head = [_lib.ptr(a), len(noff) - 1, _lib.ptr(s), 0 if s is None else len(s) - 1]
    _lib.check(L.magot_debug_orf6_tiles(*head, None, None, None, None, 0, ctypes.byref(n)),
               'tile count')
    k = n.value
    t0 = np.zeros(k + 1, np.uint64)
    r0, e0, m = (np.zeros(max(k, 1), np.uint32) for _ in range(3))
    bufs = [_lib.ptr(x) for x in (t0, r0, e0, m)]
    _lib.check(L.magot_debug_orf6_tiles(*head, *bufs, k, ctypes.byref(n)), 'tiles')
    out = []
    for i in range(k):
        t = dict(T0=int(t0[i]), T1=int(t0[i + 1]), r0=int(r0[i]))
        if s is not None:
            t.update(e0=int(e0[i]), m=int(m[i]))
        out.append(t)
    return out


def batches_of(t, noff):
    """The batch loop of one tile: per batch of 10 records each lane's lo, hi
    and cnt, n_minus, n_chunks, the segment starts in the bitmap, `more`, and
    the chunks in q order as (plus, r, f, c, p, P, rem): p the position of the
    chunk's first codon in the concatenation, P the window position of its
    lowest codon, rem the residues left in its stream."""
    n_rec = len(noff) - 1
    T0, T1, W0 = t['T0'], t['T1'], t['W0']
    rb = t['r0']
    out = []
    while True:
        lo, hi, lane_rec = [0] * SEGS, [0] * SEGS, [None] * SEGS
        for lane in range(SEGS):
            i, f = divmod(lane % (SEGS // 2), 3)
            plus = lane >= SEGS // 2
            r = rb + i
            rec = r < n_rec
            nb = noff[r] if rec else 0
            L = noff[r + 1] - nb if rec else 0
            nres = orf_count(L, f) if rec and nb < T1 else 0
            lane_rec[lane] = (plus, r, f, nb, L, nres)
            if nres:
                if plus:
                    x0 = nb + 2 * f
                    l = (T0 - x0 + 47) // 48 if T0 > x0 else 0
                    h = (T1 - x0 + 47) // 48 if T1 > x0 else 0
                else:
                    x0 = nb + L - 3 - 2 * f
                    l = (x0 - T1) // 48 + 1 if x0 >= T1 else 0
                    h = (x0 - T0) // 48 + 1 if x0 >= T0 else 0
                h = min(h, (nres + 15) // 16)
                l = min(l, h)
                lo[lane], hi[lane] = l, h
        cnt = [h - l for l, h in zip(lo, hi)]
        seg_start, chunks, acc = [], [], 0
        for lane in range(SEGS):
            if not cnt[lane]:
                continue
            seg_start.append(acc)
            acc += cnt[lane]
            plus, r, f, nb, L, nres = lane_rec[lane]
            for c in range(lo[lane], hi[lane]):
                p = nb + 2 * f + 48 * c if plus else nb + L - 3 - 2 * f - 48 * c
                chunks.append((plus, r, f, c, p, p - W0 - (0 if plus else 45), nres - 16 * c))
        r9 = rb + BATCH - 1
        more = (r9 < n_rec and noff[r9 + 1] < T1) and rb + BATCH < n_rec
        out.append(dict(rb=rb, lo=lo, hi=hi, cnt=cnt, n_minus=sum(cnt[:SEGS // 2]), n_chunks=acc,
                        seg_start=seg_start, more=more, chunks=chunks))
        if not more:
            return out
        rb += BATCH


def modes_of(b):
    """The chunk variants a batch runs, per pass of 64 chunks."""
    out = []
    for q0 in range(0, b['n_chunks'], 64):
        out.append(1 if q0 + 64 <= b['n_minus'] else 0 if q0 >= b['n_minus'] else 2)
    return out


def decompose(noff, starts=None):
    tiles = tiles_of(noff, starts)
    for t in tiles:
        t['batches'] = batches_of(t, noff)
    return tiles


def check_partition(noff, tiles):
    """Every chunk of every stream is owned by exactly one tile, the one its
    first codon starts in, and reads only what that tile staged."""
    seen = set()
    for t in tiles:
        wlen = t['WE'] - t['W0']
        for b in t['batches']:
            assert b['n_chunks'] < 32 * 128 and len(b['seg_start']) <= SEGS
            for plus, r, f, c, p, P, rem in b['chunks']:
                key = (plus, r, f, c)
                assert key not in seen, key
                seen.add(key)
                assert t['T0'] <= p < t['T1'], (key, p, t['T0'], t['T1'])
                n = min(rem, 16)
                assert n >= 1
                lo_pos = P if plus else P + 45 - 3 * (n - 1)
                hi_pos = P + 3 * n if plus else P + 48
                assert -64 <= P and 0 <= lo_pos and hi_pos <= wlen and P + 64 <= 16 * (256 + 8)
    want = set()
    for r in range(len(noff) - 1):
        for f in range(3):
            for c in range((orf_count(noff[r + 1] - noff[r], f) + 15) // 16):
                want.add((True, r, f, c))
                want.add((False, r, f, c))
    assert seen == want


# ---------------------------------------------------------------------------
# (a) lengths
# ---------------------------------------------------------------------------

def raw_case(lens, seed):
    lens = [int(x) for x in lens]
    return cut(bases(sum(lens), seed), lens)


def lengths_all():
    return raw_case(range(201), 1)


def lengths_first(L):
    """A first record of L bases, then two ordinary ones."""
    return raw_case([L, 100, 61], 100 + L)


FIRST_LENGTHS = tuple(range(3, 48))
N_RECS = tuple(range(1, 12)) + (20, 21)


def lengths_n_rec(n):
    return raw_case([30 + 7 * i for i in range(n)], 200 + n)


# ---------------------------------------------------------------------------
# (b) seams
# ---------------------------------------------------------------------------

def seams():
    """100 records of TILE + 1 bases: record i lies over seam i + 1, one base
    further in than record i - 1.  Then records ending at a seam - 1, at it and
    at it + 1, and a record longer than three tiles."""
    lens = [TILE + 1] * 100
    at = sum(lens)
    for d in (-1, 0, 1):
        want = (at // TILE + 2) * TILE + d
        lens.append(want - at)
        at = want
    lens += [3 * TILE + 100, 500]
    return raw_case(lens, 2)


def seam_cases(noff, tiles):
    """(strand, frame, phase) of every stream over a seam: the phase of the
    seam in the stream's chunks; and (strand, frame, d) for chunks whose first
    codon starts at T1 + d, d in -1, 0, 1."""
    phases, near = set(), set()
    ends = set(t['T1'] for t in tiles[:-1])
    for t in tiles:
        for b in t['batches']:
            for plus, r, f, c, p, P, rem in b['chunks']:
                for T in (t['T0'], t['T1']):
                    if T in ends and abs(p - T) <= 1:
                        near.add((plus, f, p - T))
    for r in range(len(noff) - 1):
        nb, L = noff[r], noff[r + 1] - noff[r]
        for T in ends:
            for f in range(3):
                if not orf_count(L, f):
                    continue
                x0 = nb + 2 * f
                if x0 < T < x0 + 3 * orf_count(L, f):
                    phases.add((True, f, (T - x0) % 48))
                x0 = nb + L - 3 - 2 * f
                if x0 >= T > x0 - 3 * orf_count(L, f):
                    phases.add((False, f, (x0 - T) % 48))
    return phases, near


# ---------------------------------------------------------------------------
# (c) batches
# ---------------------------------------------------------------------------

TOUCHING = (1, 9, 10, 11, 20, 21, 400)


def _group(k):
    """k records that fill one tile exactly."""
    a = TILE // k
    return [a] * (k - 1) + [TILE - a * (k - 1)]


def batches():
    """Tile-aligned groups of 1..400 records; a run of 1,000 empty records;
    three tiles whose first batch's tenth record ends at T1 - 1, T1, T1 + 1."""
    lens = []
    for k in TOUCHING:
        lens += _group(k)
    lens += [100] + [0] * 1000 + [100, TILE - 200]
    for d in (-1, 0, 1):
        lens += [300] * 9 + [TILE - 2700 + d]
        lens += [2 * TILE - (TILE + d)]       # the eleventh: up to the next seam
    return raw_case(lens, 3)


def touching(noff, t):
    return sum(1 for r in range(len(noff) - 1)
               if noff[r] < t['T1'] and noff[r + 1] > t['T0'] and noff[r + 1] > noff[r])


# ---------------------------------------------------------------------------
# (d) chunk passes
# ---------------------------------------------------------------------------

PER_STRAND = (1, 63, 64, 65, 128)


def _one_record_counts(L):
    b = decompose([0, L])[0]['batches'][0]
    return b['n_minus'], b['n_chunks'] - b['n_minus']


def find_record_length(n):
    """The first record length whose single tile owns n chunks per strand."""
    for L in range(3, TILE - 50):
        if _one_record_counts(L) == (n, n):
            return L
    raise AssertionError('no length gives %d chunks per strand' % n)


def chunk_counts(n):
    """One record, of the length found with the model for n chunks per strand
    in its one batch."""
    return raw_case([find_record_length(n)], 40 + n)


def segment_bits():
    """Groups of ten records in one tile each, chosen greedily with the model
    until the segment starts have fallen on every bit of a bitmap word, in
    words 0, 1 and beyond."""
    want = set((w, b) for w in (0, 1, 2) for b in range(32))
    have, lens = set(), []
    for k in range(400):
        g = [(17 * k + 31 * i * (k + 1)) % 380 + 3 for i in range(BATCH)]
        got = set()
        for s in decompose(offsets(g))[0]['batches'][0]['seg_start']:
            got.add((min(s >> 5, 2), s & 31))
        if got - have:
            have |= got
            lens += g + [TILE - sum(g)]
        if have >= want:
            return raw_case(lens, 5)
    raise AssertionError('segment starts never cover a bitmap word')


# ---------------------------------------------------------------------------
# (e) invalid bases
# ---------------------------------------------------------------------------

INVALID_PARTS = 2
INVALID_STEP = 97


def invalid(part):
    """Odd-length records (their starts take every phase mod 32) with one
    non-ACGT byte every 97 bases, then three clean tiles, then a dirty one."""
    lens = [1501 + 2 * ((part + i) % 5) for i in range(120)]
    lens.append(-sum(lens) % TILE + TILE)
    dirty_end = sum(lens)
    lens += [3 * TILE, 600]
    recs_total = sum(lens)
    buf = bases(recs_total, 60 + part).copy()
    at = np.arange(13 + 7 * part, dirty_end, INVALID_STEP)
    buf[at] = np.frombuffer(BAD_BYTES, np.uint8)[np.arange(len(at)) % len(BAD_BYTES)]
    buf[recs_total - 300] = ord('N')
    return cut(buf, lens)


def invalid_cases(records, tiles):
    """(strand, position of the byte in the chunk's window, P & 31) for every
    chunk with exactly one non-ACGT byte among the codons it translates; the
    tiles' tile_inv; the invalid bytes met."""
    buf = np.concatenate(records) if records else np.zeros(0, np.uint8)
    badpos = np.nonzero(~np.isin(buf, ACGT))[0]
    seen, dirty = set(), []
    for t in tiles:
        i0, i1 = np.searchsorted(badpos, [t['W0'], t['WE']])
        dirty.append(bool(i1 > i0))
        for b in t['batches']:
            for plus, r, f, c, p, P, rem in b['chunks']:
                base = P + t['W0']
                n = min(rem, 16)
                lo = base if plus else base + 48 - 3 * n
                hi = base + 3 * n if plus else base + 48
                k0, k1 = np.searchsorted(badpos, [lo, hi])
                if k1 - k0 == 1:
                    seen.add((plus, int(badpos[k0]) - base, P & 31))
    return seen, dirty, set(buf[badpos].tolist())


# ---------------------------------------------------------------------------
# (f), (g) the fused gather: contigs and tables for ExtractionPlan
# ---------------------------------------------------------------------------

G_LEN = 1 << 16
DIRTY0 = 1 << 15


def contig():
    """One contig: plain bases, then (from DIRTY0) a non-ACGT byte every 5
    bases, so that every interval of 5 bases or more there is flagged."""
    g = bases(G_LEN, 7).copy()
    at = np.arange(DIRTY0, G_LEN, 5)
    g[at] = np.frombuffer(b'NRnYK-M', np.uint8)[np.arange(len(at)) % 7]
    return g


class Fused(object):
    """Records as lists of intervals (start, length, minus) on contig(), or
    on a genome of one's own."""

    def __init__(self, records, genome=None):
        self.genome = contig() if genome is None else genome
        self.records = records
        rows, txs = [], []
        for rec in records:
            txs.append((len(rows), len(rec), 0))
            rows += [((st | RC) if minus else st, 0, ln) for st, ln, minus in rec]
        self.ex = np.array(rows, dtype=_lib.EXON_DTYPE)
        self.tx = np.array(txs, dtype=_lib.TX_DTYPE)
        # the surface orf6_windows reads
        self.contig_off = np.zeros(1, dtype=np.int64)

    def contigs(self):
        return [('c0', self.genome.tobytes())]

    def plan_tables(self):
        return self.ex, self.tx

    def record_bytes(self):
        """The records, gathered in Python (the oracle's reverse_complement)."""
        text = self.genome.tobytes().decode('latin-1')
        out = []
        for rec in self.records:
            parts = []
            for st, ln, minus in rec:
                s = text[st:st + ln]
                parts.append(mo.reverse_complement(s) if minus else s)
            out.append(np.frombuffer(''.join(parts).encode('latin-1'), np.uint8))
        return out

    def walk(self, ex_g, order):
        """The rows magot_plan_orf6 walks, from the planner's interval table
        (magot_debug_plan's ex_g: unified start | flag bits, non-empty
        intervals in record order): (perm, noff, starts, rows), rows = per
        interval (A, flagged, minus), A = anchor mod 64 of the plane position
        that walk position 0 would have."""
        iv = []
        k = 0
        for r, rec in enumerate(self.records):
            mine = []
            for st, ln, minus in rec:
                if ln:
                    g = int(ex_g[k])
                    k += 1
                    assert bool(g & RC) == bool(minus)
                    u = g & ~(RC | EXC | (1 << 61))
                    mine.append((u, ln, bool(minus), bool(g & EXC)))
            iv.append(mine)
        n = len(self.records)
        perm = list(range(n))
        if order == 'genome' and n > 1 and k:
            def key(r):
                if not iv[r]:
                    return (2, 0)
                u, ln, minus, _ = iv[r][0]
                return (1, -(u + ln)) if minus else (0, u)   # the mirror lies behind the plane
            perm.sort(key=key)
        noff, starts, rows = [0], [], []
        for r in perm:
            at = noff[-1]
            for u, ln, minus, flag in iv[r]:
                starts.append(at)
                rows.append(((-(u + ln) if minus else u) - at, flag, minus))
                at += ln
            noff.append(at)
        starts.append(noff[-1])
        return perm, noff, starts, rows


def over_genome(records):
    """Raw records as a plan: the genome is their concatenation, record r one
    interval of it, every second one on the '-' strand (the genome then holds
    its reverse complement)."""
    parts, recs, at = [], [], 0
    for r, rec in enumerate(records):
        s = rec.tobytes().decode('latin-1')
        parts.append(mo.reverse_complement(s) if r & 1 else s)
        recs.append([(at, len(rec), bool(r & 1))] if len(rec) else [])
        at += len(rec)
    genome = np.frombuffer(''.join(parts).encode('latin-1'), np.uint8)
    return Fused(recs, genome)


RAW_OVER_PLAN = dict(lengths=lengths_all, seams=seams, batches=batches)


def vectors_of(t, starts, rows):
    """The fused staging of one tile: per 16-position vector of its window
    (t, first row, j0, rows spanned); rows are window-relative."""
    e0, m, W0 = t['e0'], t['m'], t['W0']
    wlen = t['WE'] - W0
    rel = [starts[e0 + i] - W0 for i in range(m + 1)]
    assert rel[0] <= 0 and rel[m] >= wlen and m >= 1
    out = []
    i = 0
    for v in range((wlen + 15) // 16):
        t16 = 16 * v
        et = min(t16 + 16, wlen)
        while i + 1 < m and rel[i + 1] <= t16:
            i += 1
        k = 1
        while rel[i + k] < et:
            k += 1
        out.append((v, i, rel[i + 1] - t16 if k > 1 else 32, k))
    return out


def fused_cases(tiles, starts, rows):
    """What the fused staging meets: see the keys."""
    c = dict(pair=set(), a0=set(), a1=set(), shift0=set(), shift1=set(), spans=set(),
             exact=set(), m=set(), before_w0=False, only_flag=set(), capped=set())
    for t in tiles:
        e0, m, W0 = t['e0'], t['m'], t['W0']
        c['m'].add(m)
        if 'capped' in t:
            c['capped'].add(t['capped'])
        if starts[e0] < W0:
            c['before_w0'] = True
        flagged = [i for i in range(m) if rows[e0 + i][1]]
        if len(flagged) == 1:
            c['only_flag'].add(flagged[0])
        for v, i, j0, k in vectors_of(t, starts, rows):
            c['spans'].add(k)
            A0, f0, s0 = rows[e0 + i]
            if k == 2:
                A1, f1, s1 = rows[e0 + i + 1]
                c['pair'].add((j0, s0, s1, f0, f1))
                c['a0'].add((s0, (A0 + W0) & 15))
                c['a1'].add((s1, (A1 + W0) & 15))
                if f0:
                    c['shift0'].add(((A0 + W0) + 16 * v) & 31)
                if f1:
                    c['shift1'].add(((A1 + W0) + 16 * v) & 31)
            if k >= 3:
                for d in range(k):
                    A = rows[e0 + i + d][0] + W0
                    c['exact'].add((k, A & 7, (A >> 3) & 1))
    return c


def _place(a32, at, ln, minus, dirty, slot):
    """An interval of ln bases whose anchor for walk position `at` is a32 mod
    32, in the plain or in the dirty half of the contig (contig offset 0)."""
    base = (DIRTY0 if dirty else 0) + 64 + 128 * (slot % 240)
    if minus:
        end = base + 64 + ((-(a32 + at) - (base + 64)) % 32)
        return (end - ln, ln, True)
    return (base + ((a32 + at - base) % 32), ln, False)


def fused_pairs():
    """Records of 48 bases, intervals of 16 + j0 and 32 - j0: the vector at
    16..31 of every record joins two intervals at j0.  Empty records and
    records with equal keys among them."""
    recs, n, at = [], 0, 0
    for j0 in range(1, 16):
        for s0, s1 in ((0, 0), (0, 1), (1, 0), (1, 1)):
            for f0, f1 in ((0, 0), (1, 0), (0, 1), (1, 1)):
                for v in range(8):
                    a0, a1 = (7 * n + n // 32) % 32, (11 * n + 5 + n // 32) % 32
                    rec = [_place(a0, at, 16 + j0, s0, f0, n),
                           _place(a1, at + 16 + j0, 32 - j0, s1, f1, n + 1)]
                    recs.append(rec)
                    n, at = n + 1, at + 48
                    if n % 97 == 0:
                        recs.append([])                      # no interval
                        recs.append([(n, 0, False)])         # an empty one
                    if n % 131 == 0:
                        recs.append(list(rec))               # an equal key
                        at += 48
    return Fused(recs)


EXACT_SPANS = (3, 4, 16)


def fused_exact():
    """Records of 48 bases whose vector at 16..31 spans 3, 4 or 16 intervals,
    all of one anchor phase, for every phase, strand and half of the contig."""
    recs, n = [], 0
    for span in EXACT_SPANS:
        cutl = {3: [20, 5, 23], 4: [20, 5, 5, 18], 16: [17] + [1] * 14 + [17]}[span]
        for a in range(16):
            for minus in (0, 1):
                for dirty in (0, 1):
                    at, rec = 48 * n, []
                    for i, ln in enumerate(cutl):
                        rec.append(_place(a + 16 * (i & 1), at, ln, minus, dirty, 3 * n + i))
                        at += ln
                    recs.append(rec)
                    n += 1
    return Fused(recs)


ROWS_STAGED = (1, 2, 63, 64, 65, 122, 123)


def fused_rows(m, flagged=None):
    """One window of m rows of 30 bases, alternating strands; `flagged`: the
    only row taken from the dirty half."""
    rec = [_place((7 * i) % 32, 30 * i, 30, i & 1, i == flagged, i) for i in range(m)]
    return Fused([rec])


ONLY_FLAGGED = tuple(range(64, 123))


def fused_cap():
    """A record of 400 one-base intervals of alternating strand between two
    ordinary records: the row cap cuts its tiles short."""
    recs = [[(100, 700, False)],
            [(3000 + 3 * i, 1, i & 1) for i in range(400)],
            [(9000, 700, True)]]
    return Fused(recs)


def fused_edges():
    """Intervals longer than a tile (rows from before W0) on both strands, and
    intervals at the contig's first and last base, plain and flagged."""
    recs = [[(0, 40, False)], [(0, 40, True)],
            [(G_LEN - 33, 33, False)], [(G_LEN - 33, 33, True)],
            [(0, 1, False), (G_LEN - 1, 1, True), (0, 1, True), (G_LEN - 1, 1, False)],
            [(200, 3 * TILE + 77, False)], [(12345, 2 * TILE + 5, True)],
            [(DIRTY0 - 100, TILE + 300, True)], []]
    return Fused(recs)


FUSED = dict(pairs=fused_pairs, exact=fused_exact, cap=fused_cap, edges=fused_edges)
ORDERS = ('genome', 'record')
