"""mask_from_gff on the device (engine.GenomeMask, genome_tools.mask_from_gff;
maskgen.hip) against the reference's own output in
tests/golden/mask_from_gff.json and a numpy restatement (mask_expect.apply_mask)
applied to the coverage the intervals imply.  Shapes are the smallest that
reach every path of the two kernels: coverage words with every kind of edge,
text chunks at every 16-byte phase of source against destination, contigs
shorter than a chunk, and more than one block of each kernel."""

import json
import os
import subprocess
import sys

import numpy as np
import pytest

import mask_expect as me
from magot_amd import _lib, engine, genome_tools, synth

pytestmark = pytest.mark.gpu

CASES = me.load_cases()
RUNS = [(n, i) for n, i in me.all_runs(CASES)
        if CASES[n]['runs'][i]['mask_type'] in ('soft', 'hard')
        and CASES[n]['runs'][i]['overwrite_softmask'] in ('True', 'T', 'true', 't', 'TRUE') + me.KEEP]
MODES = [(False, False), (False, True), (True, False), (True, True)]  # (hard, keep_case)
# lower and upper acgtn, IUPAC in both cases, '-', '*', digits, the bytes next
# to both letter ranges, other bytes without a literal class, bytes >= 0x80
# (0xc1 / 0xe1 are 'A' / 'a' with the top bit set: no case change may touch them)
ALPHABET = np.frombuffer(b'acgtnACGTNryswkmbdhvRYSWKMBDHV-*0189@[`{ zZaA\x80\xc1\xe1\xfa\xff', np.uint8)


def gff_lines(rows):
    """(name, 0-based start, length) -> CDS lines."""
    return ''.join('%s\ts\tCDS\t%d\t%d\t.\t+\t.\tx\n' % (nm, s + 1, s + n) for nm, s, n in rows)


class Masked(object):
    """A device genome, its whole-contig extraction (executed once) and, per
    call, one mask over it."""

    def __init__(self, contigs, order=None):
        self.contigs = contigs
        self.names = [nm for nm, _ in contigs]
        self.lengths = [len(s) for _, s in contigs]
        self.dev = engine.DeviceGenome(contigs)
        self.idx = list(range(len(contigs))) if order is None else list(order)
        self.ex = engine.whole_contig_plan(self.dev, self.idx)
        self.ex.execute()
        self.lay = self.ex.layout()[0].astype(np.int64)

    def mask(self, gff, hard=False, keep_case=False):
        plan = engine.MaskPlan.build(gff, self.names, self.lengths, hard=hard, keep_case=keep_case)
        assert plan is not None, _lib.lib().magot_last_error()
        try:
            m = engine.GenomeMask(self.ex, plan, self.idx, [self.names[c] for c in self.idx])
        finally:
            plan.close()
        return m

    def expected_words(self, cov):
        """The coverage plane for one bool array per contig."""
        bits = np.zeros((self.ex.nuc_bytes + 31) // 32 * 32, bool)
        for r, c in enumerate(self.idx):
            bits[self.lay[r]:self.lay[r] + self.lengths[c]] = cov[c]
        return np.packbits(bits, bitorder='little').view('<u4')

    def expected_text(self, cov, hard, keep_case):
        return me.text_of([self.names[c] for c in self.idx],
                          [me.apply_mask(self.contigs[c][1], cov[c], hard, keep_case)
                           for c in self.idx])

    def check(self, rows, hard=False, keep_case=False, plane=True):
        cov = [np.zeros(n, bool) for n in self.lengths]
        for nm, s, n in rows:
            cov[self.names.index(nm)][s:s + n] = True
        m = self.mask(gff_lines(rows), hard, keep_case)
        try:
            m.execute()
            if plane:
                got, want = m.coverage(), self.expected_words(cov)
                bad = np.flatnonzero(got != want)
                assert len(bad) == 0, 'coverage word %d: %08x, expected %08x' % (
                    bad[0], got[bad[0]], want[bad[0]])
            text, want = m.fetch().tobytes(), self.expected_text(cov, hard, keep_case)
            assert len(text) == m.text_bytes == len(want)
            assert me.first_mismatch(text, want) is None
        finally:
            m.close()

    def close(self):
        self.ex.close()
        self.dev.close()


def draw(rng, n):
    return ALPHABET[rng.integers(0, len(ALPHABET), n)].tobytes()


@pytest.fixture(scope='module')
def plane_genome():
    rng = np.random.default_rng(7)
    g = Masked([('a', draw(rng, 261)), ('b', draw(rng, 70000)), ('c', draw(rng, 45)),
                ('d', draw(rng, 1))])
    yield g
    g.close()


def plane_sets(g):
    """name -> intervals, placed by the coverage word they fall in: `base` is
    a base of contig b at bit 0 of a word."""
    lay_b = int(g.lay[1])
    base = 64 + (-(lay_b + 64)) % 32
    assert (lay_b + base) % 32 == 0
    b = lambda s, n: ('b', base + s, n)  # noqa: E731
    return {
        'inside_one_word': [b(3, 7)],
        'ends_at_bit_31': [b(20, 12)],
        'starts_at_bit_0': [b(32, 9)],
        'bit_31_then_bit_0': [b(20, 12), b(32, 9)],
        'one_whole_word': [b(0, 32)],
        'two_whole_words': [b(0, 64)],
        'three_and_more_words': [b(5, 101), b(300, 32 * 40 + 3)],
        'duplicate_nested_abutting': [b(5, 66), b(5, 66), b(10, 11), b(71, 10), b(81, 10),
                                      b(60, 40), b(33, 31)],
        'interior_meets_edges': [b(0, 32 * 6), b(40, 5), b(64, 1), b(95, 1), b(100, 60)],
        'first_bases': [(nm, 0, 1) for nm in g.names],
        'last_bases': [(nm, n - 1, 1) for nm, n in zip(g.names, g.lengths)],
        'whole_contigs': [('c', 0, 45), ('d', 0, 1), ('a', 0, 261)],
        'whole_long_contig_in_pieces': [('b', 0, 70000)],
        'single_bases_64k': [('b', 100 + k, 1) for k in range(65536 + 300)],
        'nothing': [],
    }


PLANE_SETS = ['inside_one_word', 'ends_at_bit_31', 'starts_at_bit_0', 'bit_31_then_bit_0',
              'one_whole_word', 'two_whole_words', 'three_and_more_words',
              'duplicate_nested_abutting', 'interior_meets_edges', 'first_bases', 'last_bases',
              'whole_contigs', 'whole_long_contig_in_pieces', 'single_bases_64k', 'nothing']


@pytest.mark.parametrize('name', PLANE_SETS)
def test_coverage_plane(plane_genome, name):
    sets = plane_sets(plane_genome)
    assert sorted(sets) == sorted(PLANE_SETS)
    plane_genome.check(sets[name], hard=PLANE_SETS.index(name) % 2 == 1)


def test_needs_an_executed_extraction_and_matching_records(plane_genome):
    g = plane_genome
    fresh = engine.whole_contig_plan(g.dev, g.idx)
    plan = engine.MaskPlan.build('', g.names, g.lengths)
    try:
        m = engine.GenomeMask(fresh, plan, g.idx, g.names)
        with pytest.raises(_lib.MagotError, match='execute'):
            m.execute()
        m.close()
        with pytest.raises(_lib.MagotError, match='whole contig'):
            engine.GenomeMask(fresh, plan, [0, 1, 2, 2], g.names)
        with pytest.raises(_lib.MagotError, match='whole contig'):
            engine.GenomeMask(fresh, plan, [1, 0, 2, 3], g.names)
    finally:
        plan.close()
        fresh.close()


@pytest.fixture(scope='module')
def phase_genome():
    """51 contigs: names of 1..17 bytes against lengths 1, 15, 16, 17, 31, 33
    and 6097, in an output order other than the genome's."""
    rng = np.random.default_rng(11)
    lengths = [1, 15, 16, 17, 31, 33, 6097]
    contigs = []
    for k in range(51):
        name = ('%d_' % k + 'x' * 17)[:1 + k % 17] if k % 17 else 'abc'[k // 17]
        contigs.append((name, draw(rng, lengths[k % 7])))
    assert len({nm for nm, _ in contigs}) == 51
    g = Masked(contigs, order=[(k * 11) % 51 for k in range(51)])
    yield g
    g.close()


@pytest.mark.parametrize('hard,keep_case', MODES)
def test_text_phases_and_byte_classes(phase_genome, hard, keep_case):
    g = phase_genome
    # the bodies start at every 16-byte phase of the text
    at, phases = 0, set()
    for c in g.idx:
        at += len(g.names[c]) + 2
        phases.add(at % 16)
        at += g.lengths[c] + 1
    assert phases == set(range(16))
    rng = np.random.default_rng(13)
    rows = []
    for nm, n in zip(g.names, g.lengths):
        for _ in range(1 + n // 400):
            s = int(rng.integers(0, n))
            rows.append((nm, s, int(rng.integers(1, min(n - s, 700) + 1))))
    rows += [(g.names[3], 0, g.lengths[3]), (g.names[6], 0, 1), (g.names[6], 6096, 1)]
    g.check(rows, hard, keep_case)


@pytest.mark.parametrize('hard,keep_case', MODES)
def test_every_byte_value(hard, keep_case):
    """Every byte but CR and LF, covered and not, at every place in a word."""
    values = np.array([v for v in range(256) if v not in (10, 13)], np.uint8)
    seq = np.concatenate([np.roll(values, k) for k in range(5)])
    g = Masked([('all', seq.tobytes()), ('again', seq[::-1].tobytes())])
    try:
        g.check([('all', s, 3) for s in range(0, len(seq) - 3, 5)] + [('again', 7, 1200)],
                hard, keep_case)
    finally:
        g.close()


def _native(paths, run, order):
    return genome_tools._mask_native(paths[0], paths[1], run['mask_type'] == 'hard',
                                     run['overwrite_softmask'] in me.KEEP, run['feature_type'],
                                     order, genome_tools._Clock())


@pytest.mark.parametrize('name,i', RUNS,
                         ids=['%s-%s' % (n, me.run_id(CASES[n]['runs'][i])) for n, i in RUNS])
def test_goldens(name, i, tmp_path, capfdbinary):
    """The native path takes exactly the runs it must and prints the
    reference's bytes in both contig orders; the tool prints them too."""
    case = CASES[name]
    run = case['runs'][i]
    paths = me.case_files(case, tmp_path)
    text = _native(paths, run, 'insertion')
    if run['decline'] is not None:
        assert text is None, run['decline']
    else:
        assert text is not None
        if 'text' in run:
            assert text.tobytes().decode('latin-1') == run['text']
        assert me.sha(text) == run['sha']
        assert me.sha(_native(paths, run, 'py2')) == run['sha_py2']
    if name == 'obiroi' and i != 0:
        return  # the tool itself on the large case: once here, once in the CLI test
    exc = None
    try:
        genome_tools.mask_from_gff(paths[0], paths[1], mask_type=run['mask_type'],
                                   overwrite_softmask=run['overwrite_softmask'],
                                   feature_type=run['feature_type'])
    except Exception as e:  # noqa: BLE001
        exc = type(e).__name__
    assert exc == run['exc'] and me.sha(capfdbinary.readouterr().out) == run['sha_py2']


@pytest.fixture(scope='module')
def medium(tmp_path_factory):
    """synth at 2 Mb with its ~10^4 CDS intervals, plus a 1 Mb contig under
    one interval."""
    w = synth.make('small', genome_bases=2_000_000, n_tx=1300)
    tmp = tmp_path_factory.mktemp('mask_medium')
    contigs = w.contigs() + [('repeat1M', w.genome[:1_000_000].tobytes())]
    names = [nm for nm, _ in contigs]
    gff = w.gff3_text() + 'repeat1M\trm\tCDS\t1\t1000000\t.\t+\t.\tID=rep\n'
    rows = [(w.contig_names[int(c)], int(s), int(n))
            for c, s, n in zip(np.repeat(w.tx_contig, w.ex_count), w.ex_start, w.ex_len)]
    assert 8000 < len(rows) < 20000
    cov = {nm: np.zeros(len(s), bool) for nm, s in contigs}
    for nm, s, n in rows + [('repeat1M', 0, 1_000_000)]:
        cov[nm][s:s + n] = True
    fa, gf = str(tmp / 'm.fa'), str(tmp / 'm.gff')
    with open(fa, 'w') as fh:
        fh.write(w.fasta_text() + '>repeat1M one line\n' + contigs[-1][1].decode('latin-1') + '\n')
    with open(gf, 'w') as fh:
        fh.write(gff)
    # a slice of the first contig for the line loop: cut where no CDS lies
    first = names[0]
    cut = 200_000 + int(np.flatnonzero(~cov[first][200_000:])[0])
    sfa, sgf = str(tmp / 's.fa'), str(tmp / 's.gff')
    with open(sfa, 'w') as fh:
        fh.write('>' + first + '\n' + contigs[0][1][:cut].decode('latin-1') + '\n')
    with open(sgf, 'w') as fh:
        fh.write(gff_lines([r for r in rows if r[0] == first and r[1] + r[2] <= cut]))
    return {'fa': fa, 'gff': gf, 'contigs': contigs, 'cov': cov, 'slice': (sfa, sgf, first, cut)}


@pytest.mark.parametrize('hard,keep_case', MODES)
def test_medium_genome(medium, hard, keep_case, capfdbinary):
    names = [nm for nm, _ in medium['contigs']]
    text = genome_tools._mask_native(medium['fa'], medium['gff'], hard, keep_case, 'CDS',
                                     'insertion', genome_tools._Clock())
    assert text is not None
    text = text.tobytes()
    masked = {nm: me.apply_mask(s, medium['cov'][nm], hard, keep_case)
              for nm, s in medium['contigs']}
    want = me.text_of(names, [masked[nm] for nm in names])
    assert me.first_mismatch(text, want) is None
    assert me.sha(text) == me.sha(want)
    # the forced line loop on the slice prints what the device printed for it
    sfa, sgf, first, cut = medium['slice']
    genome_tools.mask_from_gff(sfa, sgf, mask_type='hard' if hard else 'soft',
                               overwrite_softmask='False' if keep_case else 'True',
                               native='False')
    loop = capfdbinary.readouterr().out
    assert names[0] == first
    head = len(first) + 2
    assert me.first_mismatch(loop, text[:head + cut] + b'\n') is None


def test_timing_entry_point(plane_genome):
    m = plane_genome.mask(gff_lines([('b', 5, 60000)]))
    try:
        m.execute()
        paint_ms, text_ms = m.time(2)
        assert paint_ms > 0 and text_ms > 0
    finally:
        m.close()


def test_cli_child_process(golden_dir):
    """The tool in a process of its own on the O.biroi files: its stdout is
    the golden (Python 2 order), and it took the device path."""
    case = CASES['obiroi']
    run = case['runs'][0]
    assert (run['mask_type'], run['overwrite_softmask'], run['feature_type']) == \
        ('soft', 'True', 'CDS')
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, MAGOT_CLI_TIMING='1',
               PYTHONPATH=root + os.pathsep + os.environ.get('PYTHONPATH', ''))
    res = subprocess.run([sys.executable, '-m', 'magot_amd.genome_tools', 'mask_from_gff',
                          os.path.join(golden_dir, case['fasta_file']),
                          os.path.join(golden_dir, case['gff_file'])],
                         stdout=subprocess.PIPE, stderr=subprocess.PIPE, env=env, timeout=300)
    assert res.returncode == 0, res.stderr[-2000:]
    assert me.sha(res.stdout) == run['sha_py2']
    phases = json.loads(res.stderr.decode().strip().splitlines()[-1])['cli_phases_s']
    assert 'kernels' in phases and 'text_d2h' in phases
