"""The fused longest-ORF kernel (engine.LongestOrfs) against the closed form of
tests/cdspep_expect.py: rows, flags, payload and text.  The cases are sized
from params(): S codons per step, W waves at most."""

import numpy as np
import pytest

import cdspep_expect as ce
import orfs_expect as oe
from magot_amd import _lib, engine
from oracle import magot_oracle as mo

pytestmark = pytest.mark.gpu


class Records(object):
    """Records over contigs: by default one '+' whole-contig record per
    sequence; ``recs`` = [(contig, start, length, rc)] gives others."""

    def __init__(self, seqs, recs=None, outputs=engine.OUT_NUC, execute=True):
        self.dev = engine.DeviceGenome([('c%d' % i, s) for i, s in enumerate(seqs)])
        if recs is None:
            recs = [(i, 0, len(s), False) for i, s in enumerate(seqs)]
        n = len(recs)
        ex = np.zeros(n, dtype=engine.EXON_DTYPE)
        ex['contig'] = [r[0] for r in recs]
        ex['start_rc'] = [r[1] | ((1 << 63) if r[3] else 0) for r in recs]
        ex['len'] = [r[2] for r in recs]
        tx = np.zeros(n, dtype=engine.TX_DTYPE)
        tx['exon_begin'] = np.arange(n)
        tx['n_exons'] = 1
        self.seqs = []
        for c, st, ln, rc in recs:
            s = seqs[c][st:st + ln]
            self.seqs.append(mo.reverse_complement(s) if rc else s)
        self.plan = engine.ExtractionPlan(self.dev, ex, tx, outputs)
        if execute:
            self.plan.execute()

    def close(self):
        self.plan.close()
        self.dev.close()


def check(lo, seqs, library=None):
    """The table of ``lo`` against the closed form; the expected rows."""
    rows, payload, flags = lo.table()
    want = [ce.expected_row(s, library) for s in seqs]
    assert flags.tolist() == [0 if w else _lib.ORF_REC_NO_LONGEST for w in want]
    assert rows['stream'].tolist() == [w[0] if w else 0 for w in want]
    assert rows['start'].tolist() == [w[1] if w else 0 for w in want]
    assert rows['length'].tolist() == [len(w[2]) if w else 0 for w in want]
    off = np.concatenate([[0], np.cumsum(rows['length'].astype(np.int64))])
    assert rows['payload_off'].astype(np.int64).tolist() == off[:-1].tolist()
    assert lo.payload_bytes == len(payload) == int(off[-1])
    assert payload.tobytes().decode('latin-1') == ''.join(w[2] if w else '' for w in want)
    return want


def run(seqs, recs=None, lut64=None, library=None):
    r = Records(seqs, recs)
    try:
        lo = engine.LongestOrfs(r.plan, lut64=lut64)
        try:
            return check(lo, r.seqs, library), lo.params()
        finally:
            lo.close()
    finally:
        r.close()


@pytest.fixture(scope='module')
def S():
    r = Records(['ACGTACGTAC'])
    lo = engine.LongestOrfs(r.plan)
    p = lo.params()
    lo.close()
    r.close()
    assert p['step'] >= 16 and p['waves'] >= 1 and p['max_waves'] >= p['waves']
    return p['step']


def test_every_length_and_phase():
    """Lengths 0..200 on both strands in one plan: every start phase, the None
    and empty boundaries at 2..5 bases, flagged records beside good ones."""
    contig, recs = ce.case_lengths()
    want, _ = run([contig], [(0, st, ln, rc) for st, ln, rc in recs])
    assert {st % 16 for st, _, _ in recs} == set(range(16))
    assert sum(1 for w in want if w is None) >= 6  # at least lengths 0, 1, 2 on both strands
    assert sum(1 for w in want if w) > 300


@pytest.mark.parametrize('name', ['n_lower', 'ties', 'stream_edges'])
def test_orfs_expect_cases(name):
    seqs = [s for _, s in oe.CASES[name]()]
    want, _ = run(seqs)
    if name == 'ties':  # a tie across strands: 0+ (j = 1) and 1- (j = 2) hold the maximum
        m, w = oe.longest_ties(oe.TIE_ACROSS, False)
        assert 1 in w and 2 in w and 0 not in w
        assert want[seqs.index(oe.TIE_ACROSS)][0] == 1 and len(want[seqs.index(oe.TIE_ACROSS)][2]) == m


def test_stops_around_the_step_edges(S):
    run(ce.case_step_stops(S))


def test_open_run_across_three_steps(S):
    seqs = ce.case_open_run(S)
    want, _ = run(seqs)
    for s in seqs:  # open in all six frames for three steps and more
        assert all(len(max(t.split('*'), key=len)) > 3 * S for t in oe.six_frames(s))
    assert all(len(w[2]) > 3 * S for w in want)


def test_tie_on_either_side_of_a_step_edge(S):
    seqs = ce.case_step_ties(S)
    for q, s in enumerate(seqs):
        m, tied = ce.tied_runs(s)
        assert m == S - 3 and len(tied) == 2 and tied[0][0] == tied[1][0] == (1 if q % 2 == 0 else 0)
        assert tied[0][1] // S == 0 and tied[1][1] // S == 1  # the two starts: step 0, step 1
    want, _ = run(seqs)
    for s, w in zip(seqs, want):
        assert (w[0], w[1]) == ce.tied_runs(s)[1][0]


def test_n_records():
    seqs = ce.case_n_records()
    want, _ = run(seqs)
    assert want[0] is None and want[1] is None  # NNN, NNNN
    # NNNNN: the reference keeps the 'X' behind frame 1's junk codon (get_orfs gives 'X')
    assert want[2] == (2, 0, 'X') and want[3] is not None


def test_custom_lut(S):
    lib = dict(mo.STANDARD_CODE)
    lib['GCC'] = '*'   # a stop the standard code does not have
    lib['TAA'] = 'Q'   # and one it has, read through
    lib['ATG'] = 'z'
    seqs = [s for _, s in oe.case_n_lower()] + ce.case_step_stops(S)[:4]
    want, _ = run(seqs, lut64=ce.lut64_of(lib), library=lib)
    assert want != [ce.expected_row(s) for s in seqs]


def test_more_records_than_waves():
    probe = Records(['ACGT'])
    lo = engine.LongestOrfs(probe.plan)
    W = lo.params()['max_waves']
    lo.close()
    probe.close()
    rnd = np.random.RandomState(77)
    contig = ''.join('ACGT'[i] for i in rnd.randint(0, 4, 50000))
    n = W + 67
    st = rnd.randint(0, 50000 - 64, n)
    ln = rnd.randint(0, 40, n)
    recs = [(0, int(a), int(b), bool(i & 1)) for i, (a, b) in enumerate(zip(st, ln))]
    _, p = run([contig], recs)
    assert p['waves'] == W < n


def test_genome_order_plan_gives_the_same_table():
    contig, recs = ce.case_lengths()
    recs = [(0, st, ln, rc) for st, ln, rc in recs][::-1]  # record order is not genome order
    a = Records([contig], recs)
    b = Records([contig], recs, outputs=engine.OUT_NUC | engine.OUT_GENOME_ORDER)
    try:
        assert (a.plan.layout()[0] != b.plan.layout()[0]).any()
        la, lb = engine.LongestOrfs(a.plan), engine.LongestOrfs(b.plan)
        ta, tb = la.table(), lb.table()
        check(lb, b.seqs)
        for x, y in zip(ta, tb):
            assert x.tobytes() == y.tobytes()
        la.close()
        lb.close()
    finally:
        a.close()
        b.close()


def test_text(S):
    seqs = ['NNN'] + [s for _, s in oe.case_ties()] + ce.case_n_records() + ce.case_open_run(S)
    names = ['n%d' % i for i in range(len(seqs))]
    names[1], names[2], names[3] = '', 'caf\xe9 1 two words', 'x' * 300
    r = Records(seqs)
    lo = engine.LongestOrfs(r.plan)
    try:
        for n_print in (0, 1, len(seqs), len(seqs), 5):
            got = lo.text(names, n_print).tobytes().decode('latin-1')
            assert got == ce.text_of(names, r.seqs, n_print)
        assert lo.text(names).tobytes().decode('latin-1') == ce.text_of(names, r.seqs, len(seqs))
        assert lo.time(1) > 0 and lo.time(1, text=True) > 0
        check(lo, r.seqs)  # the timed passes leave the same table
        with pytest.raises(ValueError):
            lo.text(names, len(seqs) + 1)
    finally:
        lo.close()
        r.close()


def test_refuses_a_plan_that_is_not_ready():
    r = Records(['ACGTACGTAA'], execute=False)
    try:
        with pytest.raises(_lib.MagotError, match='execute'):
            engine.LongestOrfs(r.plan)
    finally:
        r.close()
    r = Records(['ACGTACGTAA'], outputs=engine.OUT_PEP)
    try:
        with pytest.raises(_lib.MagotError, match='MAGOT_OUT_NUC'):
            engine.LongestOrfs(r.plan)
    finally:
        r.close()
