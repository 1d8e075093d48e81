"""What the interval joins must give: the reference's two predicates
(genome_tools.py:564, annotation_funcs.py:29) literally, as numpy brute force
over all pairs; the seeded worlds the device tests run on; the planner's table
restated line by line; the inputs of the recorded cases and the loader of the
reference's own results (tests/golden/overlap.json, written by
golden/make_golden_overlap.py).  Not a test module: test_overlap_host.py,
test_gpu_overlap.py and the golden generator import it."""

import json
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, 'golden')

COORD_LO, COORD_HI = -(1 << 39), (1 << 39) - 1  # what the composite key holds
NO_SEQ = 0xffffffff
REASONS = {'bad_int_first': 'bad integer in the first file',
           'bad_int_second': 'bad integer in the second file',
           'coord_range': 'coordinate beyond the key range'}


def load():
    with open(os.path.join(GOLDEN, 'overlap.json')) as fh:
        return json.load(fh)


# ---------------------------------------------------------------------------
# the predicates, over all pairs
# ---------------------------------------------------------------------------

def _pairs(iseq, p0, p1, qseq, c0, c1):
    cols = [np.asarray(x, np.int64) for x in (iseq, p0, p1, qseq, c0, c1)]
    iseq, p0, p1 = (x[None, :] for x in cols[:3])
    qseq, c0, c1 = (x[:, None] for x in cols[3:])
    return iseq == qseq, p0, p1, c0, c1


def purge_brute(iseq, p0, p1, qseq, c0, c1):
    """bool per query: genome_tools.py:564 holds for some interval of its seqid"""
    same, p0, p1, c0, c1 = _pairs(iseq, p0, p1, qseq, c0, c1)
    hit = ((p0 < c0) & (c0 < p1)) | ((p0 < c1) & (c1 < p1)) | ((c0 < p0) & (p0 < c1))
    return (hit & same).any(axis=1)


def overlap_brute(iseq, p0, p1, qseq, q0, q1):
    """int64 per query: the intervals of its seqid for which annotation_funcs.py:29 holds"""
    same, p0, p1, q0, q1 = _pairs(iseq, p0, p1, qseq, q0, q1)
    hit = ((p0 <= q0) & (q0 <= p1)) | ((p0 <= q1) & (q1 <= p1))
    return (hit & same).sum(axis=1).astype(np.int64)


# ---------------------------------------------------------------------------
# seeded worlds
# ---------------------------------------------------------------------------
# seqids: 0 dense and small-valued, 1 empty, 2 one interval, 3 and 4 neighbours
# that hold the same extreme coordinates, 5 large-valued
N_SEQ = 6
BIG = (COORD_LO, COORD_LO + 1, -(1 << 32) - 1, -(1 << 31) - 1, -(1 << 31), (1 << 31) - 1,
       1 << 31, (1 << 31) + 1, (1 << 32) - 1, 1 << 32, (1 << 32) + 1, COORD_HI - 1, COORD_HI)


def _clip(x):
    return np.clip(np.asarray(x, np.int64), COORD_LO, COORD_HI)


def index_world(n, seed=20261020):
    """(seq, p0, p1) of n intervals: the first n of one shuffled world of 4000
    that holds p1 - p0 in {-5, 0, 1, 2} many times over, 150 equal starts, 150
    equal ends, negative coordinates, the BIG ones, and the seqids above."""
    rng = np.random.default_rng(seed)
    seq, p0, p1 = [], [], []

    def add(s, a, b):
        seq.append(int(s)), p0.append(int(a)), p1.append(int(b))

    add(2, 10, 20)
    for d in (-5, 0, 1, 2):
        for a in rng.integers(-60, 300, 120):
            add(0, a, a + d)
    for b in rng.integers(60, 400, 150):  # equal starts
        add(0, 100, b)
    for a in rng.integers(-100, 240, 150):  # equal ends
        add(0, a, 200)
    for a in BIG:  # every pair of neighbouring big values, both ways, on three seqids
        for b in BIG:
            if abs(BIG.index(a) - BIG.index(b)) <= 2:
                for s in (3, 4, 5):
                    add(s, a, b)
    for s in (3, 4):  # the same extremes again, so the neighbours differ in counts only
        for _ in range(3 + s):
            add(s, COORD_LO, COORD_HI)
            add(s, COORD_HI, COORD_HI)
            add(s, COORD_LO, COORD_LO)
    while len(seq) < 4000:
        a = int(rng.integers(-80, 420))
        add(rng.choice([0, 0, 0, 5]), a, a + int(rng.integers(-8, 70)))
    order = rng.permutation(len(seq))[:n]
    return (np.asarray(seq, np.int64)[order], _clip(p0)[order], _clip(p1)[order])


def query_world(iseq, p0, p1, n=3000, seed=20261021):
    """(seq, c0, c1) of about n queries against that index: c0 and c1 each at
    p0 - 1, p0, p0 + 1, p1 - 1, p1, p1 + 1 of picked intervals in all 36
    combinations (c0 > c1 and c0 == c1 among them), the BIG coordinates, random
    small ones, every seqid, and two the index does not hold."""
    rng = np.random.default_rng(seed)
    seq, c0, c1 = [], [], []
    if len(iseq):
        picks = rng.choice(len(iseq), size=min(len(iseq), 45), replace=False)
        for k in picks:
            edges = [p0[k] - 1, p0[k], p0[k] + 1, p1[k] - 1, p1[k], p1[k] + 1]
            for a in edges:
                for b in edges:
                    seq.append(iseq[k]), c0.append(a), c1.append(b)
    for s in (3, 4, 5, 1):
        for a in BIG:
            for b in (a, COORD_LO, COORD_HI, a + 1, a - 1):
                seq.append(s), c0.append(a), c1.append(b)
    while len(seq) < n:
        a = int(rng.integers(-90, 430))
        seq.append(int(rng.choice([0, 0, 0, 0, 1, 2, 5, -1, N_SEQ + 3])))
        c0.append(a), c1.append(a + int(rng.integers(-10, 80)))
    return np.asarray(seq, np.int64), _clip(c0), _clip(c1)


def range_world(counts, seed=20261022):
    """An index and one query per entry of ``counts``: on seqid k exactly
    counts[k] intervals start inside the query (1000, 5000], about half of
    them ending at or past its end; some start at or before 1000 and some
    after 5000.  Returns (index columns, query columns)."""
    rng = np.random.default_rng(seed)
    seq, p0, p1 = [], [], []
    for k, m in enumerate(counts):
        starts = rng.integers(1001, 5001, m)
        if m:
            starts[0], starts[-1] = 1001, 5000
        for a in starts:
            seq.append(k), p0.append(a)
            p1.append(int(rng.choice([a, 4999, 5000, 5001, 9000])))
        for a, b in ((1000, 5000), (1000, 999), (900, 1000), (900, 7000), (5001, 6000),
                     (1000, 1000)):
            seq.append(k), p0.append(a), p1.append(b)
    order = rng.permutation(len(seq))
    index = tuple(np.asarray(x, np.int64)[order] for x in (seq, p0, p1))
    ks = np.arange(len(counts), dtype=np.int64)
    # each range asked as (lo, hi) and as (hi, lo)
    query = (np.concatenate([ks, ks]),
             np.concatenate([np.full(len(ks), 1000), np.full(len(ks), 5000)]).astype(np.int64),
             np.concatenate([np.full(len(ks), 5000), np.full(len(ks), 1000)]).astype(np.int64))
    return index, query


# ---------------------------------------------------------------------------
# the planner's table, restated
# ---------------------------------------------------------------------------
_SPACE = b' \t\n\r\x0b\x0c'


class Decline(Exception):
    pass


def _int(field, first):
    s = field.strip(_SPACE)
    digits = s[1:] if s[:1] in (b'+', b'-') else s
    if not digits or not digits.isdigit():
        raise Decline(REASONS['bad_int_first' if first else 'bad_int_second'])
    v = int(s)
    if len(digits) > 18 or not COORD_LO <= v <= COORD_HI:
        raise Decline(REASONS['coord_range'])
    return v


def file_lines(data):
    """Python 2's ``for line in file``: lines end after LF only"""
    lines = data.split(b'\n')
    return [ln + b'\n' for ln in lines[:-1]] + ([lines[-1]] if lines[-1] else [])


def plan_tables(first, second):
    """([table of file 0, table of file 1], n_seq), each table a dict of lists
    'flag', 'seq', 'c0', 'c1', 'off', 'len' with one entry per line; raises
    Decline(reason) where magot_overlap_plan declines."""
    seq_of = {}
    tables = []
    for which, data in enumerate((first, second)):
        t = {k: [] for k in ('flag', 'seq', 'c0', 'c1', 'off', 'len')}
        at = 0
        for line in file_lines(data):
            flag = line.count(b'\t') > 6
            seq, c0, c1 = NO_SEQ, 0, 0
            if flag:
                x = line.split(b'\t')
                if which == 0 or x[0] in seq_of:
                    c0, c1 = _int(x[3], which == 0), _int(x[4], which == 0)
                    seq = seq_of.setdefault(x[0], len(seq_of))
            for k, v in zip(('flag', 'seq', 'c0', 'c1', 'off', 'len'),
                            (int(flag), seq, c0, c1, at, len(line))):
                t[k].append(v)
            at += len(line)
        tables.append(t)
    return tables, len(seq_of)


def purge_expected(first, second):
    """purge_overlaps' stdout bytes for two texts the planner accepts, from the
    tables and the brute force"""
    (t0, t1), _ = plan_tables(first, second)
    rows = [k for k, f in enumerate(t0['flag']) if f]
    drop = purge_brute([t0['seq'][k] for k in rows], [t0['c0'][k] for k in rows],
                       [t0['c1'][k] for k in rows], t1['seq'], t1['c0'], t1['c1'])
    out = []
    for k, line in enumerate(file_lines(second)):
        if t1['flag'][k] and not (t1['seq'][k] != NO_SEQ and drop[k]):
            out.append(line[:-1] + b'\n')
    return b''.join(out)


# ---------------------------------------------------------------------------
# the recorded cases' inputs
# ---------------------------------------------------------------------------

def gff_line(seqid, a, b, tail=b'.\t+\t.\tID=x', eol=b'\n'):
    """A line with 8 tabs unless ``tail`` says otherwise"""
    def enc(v):
        return v if isinstance(v, bytes) else str(v).encode()
    return enc(seqid) + b'\tsrc\tgene\t' + enc(a) + b'\t' + enc(b) + b'\t' + tail + eol


def purge_cases():
    """name -> (first file, second file, expected path: 'native' or the
    decline reason)"""
    g = gff_line
    c = {}
    # every strictness edge: c0 and c1 each at the six positions around (100, 200)
    edges = (99, 100, 101, 199, 200, 201)
    c['edges'] = (g('a', 100, 200), b''.join(g('a', x, y) for x in edges for y in edges), 'native')
    c['edges_widths'] = (b''.join(g('a', 50, 50 + d) for d in (-5, 0, 1, 2)),
                         b''.join(g('a', x, y) for x in range(43, 55) for y in (x, x + 1, x + 3)),
                         'native')
    c['contains_end_not_start'] = (g('a', 100, 200), g('a', 150, 300) + g('a', 200, 300) +
                                   g('a', 99, 150) + g('a', 100, 200) + g('a', 99, 201), 'native')
    c['reversed_and_negative'] = (g('a', 200, 100) + g('a', -50, -10) + g('b', -5, 5),
                                  g('a', 150, 150) + g('a', 250, 50) + g('a', 50, 250) +
                                  g('a', -30, -20) + g('a', -60, -40) + g('a', -10, -50) +
                                  g('b', 0, 0) + g('b', 5, -5) + g('b', -6, 6), 'native')
    c['tabs_6_and_7'] = (g('a', 100, 200, tail=b'.\t+\t.') + g('a', 300, 400, tail=b'.\t+'),
                         g('a', 150, 160, tail=b'.\t+\t.') + g('a', 150, 160, tail=b'.\t+') +
                         g('a', 350, 360, tail=b'.\t+\t.') + g('a', 350, 360, tail=b'.\t+'),
                         'native')
    c['hash_lines'] = (b'#a\ts\tt\t100\t200\t.\t+\t.\tx\n' + b'# a comment\n',
                       b'#a\ts\tt\t150\t160\t.\t+\t.\tx\n#a\ts\tt\t300\t400\t.\t+\t.\n' +
                       b'##gff-version 3\n#a\ts\tt\tx\ty\t.\t+\n', 'native')
    c['unknown_seqid_bad_integers'] = (g('a', 100, 200), g('zz', b'x', b'') + g('zz', 150, 160) +
                                       g('a', 150, 160) + g('A', 150, 160), 'native')
    c['bad_integer_first'] = (g('a', 100, 200) + g('a', b'1e3', 5), g('a', 1, 2), 'bad_int_first')
    c['bad_integer_second'] = (g('a', 100, 200),
                               g('a', 1, 2) + g('a', 150, 160) + g('b', 150, 160) +
                               g('a', 300, b'4 0') + g('a', 5, 6), 'bad_int_second')
    c['bad_integer_second_few_tabs'] = (g('a', 100, 200), g('a', b'x', b'y', tail=b'.\t+') +
                                        g('a', 500, 600), 'native')
    c['python_int_forms'] = (g('a', b' +100 ', b'\x0b200\x0c'), g('a', b'-0', b'+150') +
                             g('a', b' 300', b'400 '), 'native')
    c['long_integers'] = (g('a', 100, 10 ** 20), g('a', 10 ** 19, 10 ** 19 + 5) + g('a', 1, 2),
                          'coord_range')
    c['crlf'] = (g('a', 100, 200, eol=b'\r\n'),
                 g('a', 150, 160, eol=b'\r\n') + g('a', 300, 400, eol=b'\r\n') + b'\r\n' +
                 g('a', 300, 400, tail=b'.\t+\t.', eol=b'\r\n'), 'native')
    c['no_final_lf'] = (g('a', 100, 200)[:-1], g('a', 150, 160) + g('a', 300, 400)[:-1], 'native')
    c['no_final_lf_dropped'] = (g('a', 100, 200), g('a', 300, 400) + g('a', 150, 160)[:-1],
                                'native')
    c['no_final_lf_short'] = (g('a', 100, 200), g('a', 300, 400) + b'x', 'native')
    c['empty_first'] = (b'', g('a', 150, 160) + b'\n' + b'text\n', 'native')
    c['empty_second'] = (g('a', 100, 200), b'', 'native')
    c['empty_both'] = (b'', b'', 'native')
    c['only_lfs'] = (b'\n\n', b'\n\n\n', 'native')
    c['duplicate_lines'] = (g('a', 100, 200) * 3 + g('b', 1, 9) * 2,
                            (g('a', 150, 160) + g('a', 300, 400) + g('b', 5, 6)) * 3, 'native')
    c['several_seqids'] = (g('a', 100, 200) + g('b', 1000, 2000) + g('c', 5, 5) + g('a', 400, 500),
                           b''.join(g(s, x, x + 30) for s in ('a', 'b', 'c', 'd')
                                    for x in (80, 180, 380, 480, 980, 1980, 2000, 5)), 'native')
    c['big_coordinates'] = (g('a', (1 << 31) - 1, (1 << 32) + 1) + g('b', COORD_LO, COORD_HI),
                            g('a', 1 << 31, 1 << 31) + g('a', (1 << 32) + 1, (1 << 32) + 2) +
                            g('a', (1 << 32), 1 << 33) + g('b', COORD_LO, COORD_LO + 1) +
                            g('b', COORD_HI - 1, COORD_HI) + g('b', COORD_LO + 1, COORD_LO + 1),
                            'native')
    rng = np.random.default_rng(20261020)
    for k in range(6):
        files = []
        for n in (int(rng.integers(0, 25)), int(rng.integers(0, 60))):
            lines = []
            for _ in range(n):
                a = int(rng.integers(-20, 300))
                lines.append(g(rng.choice(['a', 'b', 'c']), a, a + int(rng.integers(-10, 60)),
                               tail=rng.choice([b'.\t+\t.\tID=x', b'.\t+\t.', b'.\t+'])))
            files.append(b''.join(lines))
        c['random_%02d' % k] = (files[0], files[1], 'native')
    return c


def overlap_cases():
    """name -> two annotation sets and the feature dicts to compare.  A set is
    {'CDS': [[ID, seqid, c0, c1], ...], 'transcript': [[ID, seqid, [children]],
    ...], 'gene': the same}"""
    c = {}
    one = {'CDS': [['p1', 'a', 100, 200], ['p2', 'a', 150, 250], ['p3', 'a', 190, 195],
                   ['p4', 'b', 100, 200], ['p5', 'a', 300, 300]]}
    two = {'CDS': [['q_three', 'a', 192, 194], ['q_touch_start', 'a', 50, 100],
                   ['q_touch_end', 'a', 250, 260], ['q_contains', 'a', 90, 260],
                   ['q_miss', 'a', 260, 299], ['q_point', 'a', 300, 300],
                   ['q_other_seqid', 'b', 150, 150], ['q_unknown_seqid', 'zz', 150, 150],
                   ['q_reversed', 'a', 260, 150]]}
    c['base_features'] = (one, 'CDS', two, 'CDS')
    genes = {'CDS': [['c1', 'a', 100, 150], ['c2', 'a', 300, 350], ['c3', 'a', 1000, 1100],
                     ['c4', 'b', 10, 20], ['c5', 'a', 120, 130]],
             'transcript': [['t1', 'a', ['c1', 'c2']], ['t2', 'a', ['c3']], ['t3', 'b', ['c4']],
                            ['t4', 'a', ['c5']]],
             'gene': [['g1', 'a', ['t1', 't4']], ['g2', 'a', ['t2']], ['g3', 'b', ['t3']]]}
    c['genes_against_cds'] = (genes, 'gene', two, 'CDS')
    c['cds_against_genes'] = (one, 'CDS', genes, 'gene')
    c['transcripts_against_transcripts'] = (genes, 'transcript', genes, 'transcript')
    childless = {'CDS': [['c1', 'a', 100, 150]],
                 'transcript': [['t1', 'a', ['c1']], ['t_empty', 'a', []]]}
    c['childless_parent_first'] = (childless, 'transcript', two, 'CDS')
    c['childless_parent_second'] = (one, 'CDS', childless, 'transcript')
    c['childless_parent_unknown_seqid'] = (
        one, 'CDS', {'CDS': [], 'transcript': [['t_empty', 'zz', []]]}, 'transcript')
    c['empty_first'] = ({'CDS': []}, 'CDS', two, 'CDS')
    c['empty_second'] = (one, 'CDS', {'CDS': []}, 'CDS')
    many = {'CDS': [['m%d' % k, 'ab'[k % 2], 10 * k, 10 * k + 25] for k in range(40)]}
    c['many'] = (many, 'CDS', many, 'CDS')
    return c


def build_features(module, spec, which):
    """The feature dict ``which`` of an annotation set made from ``spec`` with
    ``module``'s classes (the package's genome module, or the reference's)"""
    aset = module.AnnotationSet()
    for row in spec.get('CDS', []):
        aset.CDS[row[0]] = module.BaseAnnotation(row[0], row[1], (row[2], row[3]), 'CDS',
                                                 annotation_set=aset)
    for kind in ('transcript', 'gene'):
        for row in spec.get(kind, []):
            getattr(aset, kind)[row[0]] = module.ParentAnnotation(row[0], row[1], kind,
                                                                   child_list=row[2],
                                                                   annotation_set=aset)
    return getattr(aset, which)
