"""ORF calling on the device (engine.OrfCalls, genome_tools.dna2orfs) against
the closed form of tests/orfs_expect.py and the reference's own output in
tests/golden/dna2orfs.json.  The inputs are the smallest that reach every
path of the kernels: see orfs_expect.CASES (tile size engine.ORFCALL_TILE)."""

import json
import os

import numpy as np
import pytest

import orfs_expect as oe
from magot_amd import _lib, engine, genome_tools, synth
from oracle import magot_oracle as mo

pytestmark = pytest.mark.gpu

TABLE_CASES = sorted(oe.CASES)


@pytest.fixture(scope='module')
def golden(golden_dir):
    with open(os.path.join(golden_dir, 'dna2orfs.json')) as fh:
        return json.load(fh)['cases']


class Calls(object):
    """One '+' whole-contig record per contig -> Orf6Plan -> OrfCalls per mode."""

    def __init__(self, contigs):
        self.contigs = contigs
        self.dev = engine.DeviceGenome(contigs)
        n = len(contigs)
        ex = np.zeros(n, dtype=engine.EXON_DTYPE)
        ex['contig'] = np.arange(n)
        ex['len'] = [len(s) for _, s in contigs]
        tx = np.zeros(n, dtype=engine.TX_DTYPE)
        tx['exon_begin'] = np.arange(n)
        tx['n_exons'] = 1
        self.plan = engine.ExtractionPlan(self.dev, ex, tx, engine.OUT_NUC)
        self.o6 = engine.Orf6Plan(self.plan)
        self.o6.execute()

    def close(self):
        self.o6.close()
        self.plan.close()
        self.dev.close()


def expected_table(seqs, from_atg, longest):
    """(rows [(record, j, k, output)], flags) the device table must hold."""
    rows, flags = [], []
    for r, seq in enumerate(seqs):
        got, none_j = oe.contig_rows(seq, from_atg)
        flag = _lib.ORF_REC_NONE if none_j is not None else 0
        if longest:
            best = oe.longest_row(got)
            if not flag and best is None:
                flag = _lib.ORF_REC_NO_LONGEST
            got = [best] if not flag else []
        flags.append(flag)
        rows += [(r, j, k, out) for j, k, _, out in got]
    return rows, flags


def check_table(calls, seqs, from_atg, longest):
    rows, payload, flags = calls.table()
    want, want_flags = expected_table(seqs, from_atg, longest)
    assert flags.tolist() == want_flags
    assert calls.n_orfs == len(rows) == len(want)
    assert rows['record'].tolist() == [w[0] for w in want]
    assert rows['stream'].tolist() == [w[1] for w in want]
    assert rows['start'].tolist() == [w[2] for w in want]
    assert rows['length'].tolist() == [len(w[3]) for w in want]
    off = np.concatenate([[0], np.cumsum(rows['length'].astype(np.int64))])
    assert rows['payload_off'].astype(np.int64).tolist() == off[:-1].tolist()
    assert calls.payload_bytes == len(payload) == int(off[-1])
    assert payload.tobytes().decode('latin-1') == ''.join(w[3] for w in want)
    return sum(1 for f in want_flags if f)


@pytest.mark.parametrize('name', TABLE_CASES)
def test_table_and_text(name):
    """Table parity and text parity against the helper, all four modes."""
    assert oe.TILE == engine.ORFCALL_TILE
    contigs = oe.CASES[name]()
    names = [nm for nm, _ in contigs]
    seqs = [s for _, s in contigs]
    c = Calls(contigs)
    try:
        for from_atg, longest in oe.MODES:
            calls = engine.OrfCalls(c.o6, from_atg=from_atg, longest=longest)
            try:
                n_flagged = check_table(calls, seqs, from_atg, longest)
                # flagged records: short1..4 hold exactly one each, nothing else any
                assert n_flagged == (1 if name.startswith('short') else 0)
                text = calls.text(names).tobytes().decode('latin-1')
                # a flagged record's block is what the reference wrote before it
                # failed (default), or nothing (longest)
                want = ''.join(oe.block(nm, s, from_atg, longest)[0] for nm, s in contigs)
                assert text == want
                assert calls.time(1) > 0 and calls.time(1, text=True) > 0
                assert calls.text(names).tobytes().decode('latin-1') == want  # passes re-run
            finally:
                calls.close()
    finally:
        c.close()


def test_needs_an_executed_plan():
    c = Calls(oe.case_ties())
    try:
        fresh = engine.Orf6Plan(c.plan)
        with pytest.raises(_lib.MagotError, match='execute'):
            engine.OrfCalls(fresh)
        fresh.close()
    finally:
        c.close()


def test_longest_ties_follow_loop_order():
    """The maximum lies in 0+ (j = 1) and 1- (j = 2); 1- comes first in memory."""
    contigs = oe.case_ties()
    c = Calls(contigs)
    try:
        for from_atg, seq_across in ((False, oe.TIE_ACROSS), (True, oe.TIE_ACROSS_ATG)):
            m, w = oe.longest_ties(seq_across, from_atg)
            assert 1 in w and 2 in w and 0 not in w
            calls = engine.OrfCalls(c.o6, from_atg=from_atg, longest=True)
            rows, _, _ = calls.table()
            calls.close()
            r = [s for _, s in contigs].index(seq_across)
            assert int(rows['stream'][r]) == 1 and int(rows['length'][r]) == m
        soff, _ = c.o6.fetch_to(None)
        assert int(soff[2]) < int(soff[1])  # memory order: 1- before 0+
    finally:
        c.close()


def run_tool(tmp_path, fasta_text, from_atg, longest, extra=()):
    fa = tmp_path / 'in.fa'
    out = tmp_path / 'out.fa'
    fa.write_bytes(fasta_text.encode('latin-1'))
    if out.exists():
        out.unlink()
    argv = ['dna2orfs', str(fa), str(out)]
    argv += ['from_atg=1'] if from_atg else []
    argv += ['longest=1'] if longest else []
    exc = None
    try:
        assert genome_tools.main(argv + list(extra)) == 0
    except (AttributeError, IndexError) as e:
        exc = type(e).__name__
    return out.read_bytes().decode('latin-1'), exc


@pytest.mark.parametrize('name', TABLE_CASES + ['obiroi'])
def test_dna2orfs_end_to_end(name, golden, golden_dir, tmp_path):
    """main([...]) into a file against the reference's recorded output, in
    Python 2 dict order (the default) and in insertion order; short contigs
    take the declining path: the reference's exception and partial file."""
    case = golden[name]
    if 'input_file' in case:
        with open(os.path.join(golden_dir, case['input_file']), encoding='latin-1',
                  newline='') as fh:
            text = fh.read()
    else:
        text = oe.fasta(oe.CASES[name]())
    assert oe.sha(text) == case['input_sha']
    for from_atg, longest in oe.MODES:
        want = case['modes']['%d%d' % (from_atg, longest)]
        got, exc = run_tool(tmp_path, text, from_atg, longest, ['order=insertion'])
        assert (oe.sha(got), exc) == (want['sha'], want['exc'])
        if 'text' in want:
            assert got == want['text']
        got, exc = run_tool(tmp_path, text, from_atg, longest)
        assert (oe.sha(got), exc) == (want['sha_py2'], want['exc_py2'])
    if name.startswith('short'):
        assert want['exc'] == 'AttributeError'
    if name == 'names':  # the two orders differ on these names
        assert case['modes']['00']['sha'] != case['modes']['00']['sha_py2']


def test_host_loop_equals_native(golden, tmp_path):
    text = oe.fasta(oe.case_all_lengths())
    for from_atg, longest in oe.MODES:
        want = golden['all_lengths']['modes']['%d%d' % (from_atg, longest)]
        native, exc = run_tool(tmp_path, text, from_atg, longest)
        assert exc is None and oe.sha(native) == want['sha_py2']
        host, exc = run_tool(tmp_path, text, from_atg, longest, ['native=False'])
        assert exc is None and host == native


def test_native_path_is_taken_and_declines(tmp_path, monkeypatch):
    """The device path serves the unflagged inputs; a flagged one declines."""
    calls = []
    real = genome_tools._dna2orfs_native

    def spy(*args):
        res = real(*args)
        calls.append(res is not None)
        return res

    monkeypatch.setattr(genome_tools, '_dna2orfs_native', spy)
    ties = oe.case_ties()
    native, _ = run_tool(tmp_path, oe.fasta(ties), False, False)
    _, exc = run_tool(tmp_path, oe.fasta(oe.case_short(4)), False, False)
    assert calls == [True, False] and exc == 'AttributeError'
    # a genome above one device plane declines too, and the loop writes the same
    monkeypatch.setattr(engine, 'PART_BASES', 100)
    host, exc = run_tool(tmp_path, oe.fasta(ties), False, False)
    assert calls == [True, False, False] and exc is None and host == native
    monkeypatch.undo()
    monkeypatch.setattr(genome_tools, '_dna2orfs_native', spy)
    # names are bytes to the device: one with a byte >= 0x80 is served there
    odd = [('caf\xe9 1', ties[0][1]), ('plain', ties[2][1])]
    for order in ('py2', 'insertion'):
        got, exc = run_tool(tmp_path, oe.fasta(odd), True, False, ['order=' + order])
        assert (got, exc) == oe.tool_text(odd, True, False, order=order)
    assert calls == [True, False, False, True, True]


def test_records_that_are_not_whole_contigs():
    """The small synthetic workload's spliced records: the table is in record
    order although the six-frame kernel lays the records out in genome order,
    and equals Sequence.get_orfs per record once the rows of empty streams
    (which get_orfs skips) are dropped."""
    w = synth.make('small', seed=43, genome_bases=1_000_000, n_tx=60, iupac_rate=2e-3)
    dev = engine.DeviceGenome(w.contigs())
    ex, tx = w.plan_tables()
    plan = engine.ExtractionPlan(dev, ex, tx, engine.OUT_NUC)
    nuc, noff, _, _ = plan.run()
    o6 = engine.Orf6Plan(plan)
    o6.execute()
    try:
        soff, _ = o6.fetch_to(None)
        blocks = soff[:-1:6].astype(np.int64)
        assert (np.diff(blocks) < 0).any()  # device layout is not record order
        raw = nuc.tobytes().decode('latin-1')
        seqs = [raw[int(noff[r]):int(noff[r + 1])] for r in range(len(tx))]
        assert min(len(s) for s in seqs) > 4
        for from_atg in (False, True):
            calls = engine.OrfCalls(o6, from_atg=from_atg)
            rows, payload, flags = calls.table()
            calls.close()
            assert not flags.any()
            assert (np.diff(rows['record'].astype(np.int64)) >= 0).all()
            pay = payload.tobytes().decode('latin-1')
            dropped = want_dropped = 0
            for r, seq in enumerate(seqs):
                six = oe.six_frames(seq)
                want_dropped += sum(1 for t in six if t == '')
                got = []
                for row in rows[rows['record'] == r]:
                    if six[int(row['stream'])] == '':
                        dropped += 1
                        continue
                    o = int(row['payload_off'])
                    got.append(pay[o:o + int(row['length'])])
                assert got == mo.get_orfs(seq, from_atg=from_atg)
            assert dropped == want_dropped
            calls = engine.OrfCalls(o6, from_atg=from_atg, longest=True)
            rows, payload, flags = calls.table()
            calls.close()
            assert not flags.any() and rows['record'].tolist() == list(range(len(seqs)))
            pay = payload.tobytes().decode('latin-1')
            for r, seq in enumerate(seqs):
                o = int(rows['payload_off'][r])
                assert pay[o:o + int(rows['length'][r])] == \
                    mo.get_orfs(seq, longest=True, from_atg=from_atg)
    finally:
        o6.close()
        plan.close()
        dev.close()
