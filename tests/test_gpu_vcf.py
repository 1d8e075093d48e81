"""heterozygosity_from_vcf on the device (vcf.hip; magot_variants.py:16-139):
engine.VariantHets' tables (positions, key hashes, het bit rows, kept and first
flags, counts per locus) against the restated model of vcf_expect.py on seeded
worlds, exactly; every run recorded from the reference through
magot_variants.heterozygosity_from_vcf on both paths and in both orders, each
decline with its named reason; the limits; one command-line call.

Worlds: every line count (1, around a wave and around a workgroup of data
lines, 4099: the sort and the line index then span several blocks) at 3
samples, every sample count (around one and two bit words, 130) at 257 lines,
and 4099 x 65."""

import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

import vcf_expect as ve
from magot_amd import engine, genome_tools, magot_variants

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = ve.load()
NAMES = sorted(GOLD)


def _native(text, **kw):
    """engine.VariantHets of a text that must not be declined"""
    hets = engine.VariantHets.parse(text.encode('latin-1'), **kw)
    assert isinstance(hets, engine.VariantHets), (hets, engine.VariantHets.last_declined_line)
    return hets


def _words(bits, words):
    """model bit rows (Python ints) as n x words uint32"""
    return np.array([[b >> (32 * w) & 0xffffffff for w in range(words)] for b in bits], np.uint32)


def _spans(text, off, length):
    return [text[int(o):int(o) + int(n)] for o, n in zip(off.tolist(), length.tolist())]


def _locus_columns(loci, ids=None):
    """``ids``: the contig id of every name; without it the names are numbered
    as the loci bring them"""
    contig, lo, hi = [], [], []
    if ids is None:
        ids = {}
        for locus in loci:
            ids.setdefault(locus.split(',')[0], len(ids))
    for locus in loci:
        f = locus.split(',')
        contig.append(ids[f[0]])
        a, b = (int(f[1]), int(f[2])) if len(f) > 2 else (0, 2 ** 32 - 1)
        a, b = max(a, 0), min(b, 2 ** 32 - 1)
        lo.append(a if a <= b else 1)
        hi.append(b if a <= b else 0)
    return ids, contig, lo, hi


def _assert_equals_table(hets, text, loci, order, ids=None):
    want = ve.table(text, loci, order, ids)
    n = len(want['line'])
    assert (hets.n_data, hets.n_runs) == (n, len(want['runs']))
    lines = ve.split_lines(text)
    assert hets.n_lines == len(lines)
    assert hets.n_header == sum(ln[:2] == '##' for _, ln in lines)
    assert _spans(text, *hets.header_lines()) == [ln for _, ln in lines if ln[:2] == '##']
    assert text[hets.header[0]:sum(hets.header)] == [ln for _, ln in lines
                                                     if ln[:1] == '#' and ln[:2] != '##'][0]
    assert _spans(text, *hets.runs()) == want['runs']
    ids, contig, lo, hi = _locus_columns(loci, ids)
    hets.resolve([ids[name] for name in want['runs']])
    t = hets.tables()
    assert t['bits'].shape == (n, hets.words) and hets.words == (hets.n_samples + 31) // 32
    for name in ('line', 'pos', 'hash', 'kept', 'first'):
        assert t[name].tolist() == want[name], name
    assert (t['bits'] == _words(want['bits'], hets.words)).all()
    line, off, length = hets.first_variant_line(order)
    assert line == want['first_line'] and text[off:off + length] == lines[line][1]
    allowed = _words([want['allowed']], hets.words)[0]
    counts, foreign = hets.count(contig, lo, hi, allowed)
    assert counts.dtype == np.uint32 and counts.tolist() == want['counts']
    assert foreign == want['foreign']
    # with every column allowed nothing is foreign, and the counts stand
    counts, foreign = hets.count(contig, lo, hi, np.full(hets.words, 0xffffffff, np.uint32))
    assert counts.tolist() == want['counts'] and not foreign
    return want


@pytest.mark.parametrize('n_data,n_samples', ve.WORLDS, ids=['%dx%d' % w for w in ve.WORLDS])
def test_tables_equal_the_restated_model(n_data, n_samples):
    text, loci = ve.world(n_data, n_samples)
    hets = _native(text)
    try:
        assert (hets.n_data, hets.n_samples) == (n_data, n_samples)
        _assert_equals_table(hets, text, loci, 'py2' if n_data % 2 else 'insertion')
    finally:
        hets.close()


def test_the_worlds_hold_what_they_promise():
    assert {n for n, s in ve.WORLDS if s == 3} == set(ve.LINE_COUNTS)
    assert {s for n, s in ve.WORLDS if n == 257} == set(ve.SAMPLE_COUNTS) | {3}
    assert (4099, 65) in ve.WORLDS
    for n_data, n_samples in ve.WORLDS:
        text, loci = ve.world(n_data, n_samples)
        assert ve.native_note(text, loci) in ('native', 'foreign_name')
        lines = [ln for _, ln in ve.split_lines(text)]
        starts = np.cumsum([0] + [len(ln) + 1 for ln in lines])
        assert (starts[1:-1] % ve.TEXT_BLOCK == 0).any()  # an LF ends a block, a line starts one
        assert max(len(ln) for ln in lines) > 8192
        t = ve.table(text, loci, 'py2')
        assert len(t['line']) == n_data and len(t['runs']) == min(n_data, 4)
        if n_data < 63:
            continue
        assert 0 < sum(t['kept']) < n_data  # keys repeat
        data = [ln.split('\t') for ln in lines if ln[:1] != '#']
        if n_samples > 1:
            assert any(f.index(c) != 9 + s for f in data for s, c in enumerate(f[9:]))
        assert any(t['bits']) and any(f[8] == 'DP:GT' for f in data)
        whole = [sum(f[0] == locus.split(',')[0] for f in data)
                 for locus in loci if len(locus.split(',')) == 2]
        assert (max(whole) > engine.VariantHets.params()[0]) == (n_data == 4099)  # the pieces' atomics meet
        assert 0 in [sum(row) for row in t['counts']] and max(map(max, t['counts'])) > 1


# ---------------------------------------------------------------------------
# the recorded runs
# ---------------------------------------------------------------------------

def _run(fn, capfd):
    ret = exc = None
    try:
        ret = fn()
    except Exception as e:  # noqa: BLE001
        exc = type(e).__name__
    return capfd.readouterr().out, ret, exc


def test_at_most_half_of_the_goldens_leave_the_device_path():
    notes = [GOLD[n][o]['note'] for n in NAMES for o in ve.ORDERS]
    assert sum(note != 'native' for note in notes) * 2 <= len(notes)
    assert {'raise', 'foreign_name', 'carriage_return', 'duplicate_names', 'locus_form',
            'header_form'} <= set(notes)
    parse_reasons = set(engine._lib.VCF_REASONS[1:]) - {
        'too_many_samples', 'too_large', 'too_many_lines', 'too_many_runs', 'line_too_long',
        'too_many_counts', 'no_samples'}
    assert parse_reasons <= set(notes)


@pytest.mark.parametrize('name', NAMES)
def test_goldens_on_both_paths_in_both_orders(name, tmp_path, capfd):
    case = GOLD[name]
    path = str(tmp_path / 'calls.vcf')
    with open(path, 'wb') as fh:
        fh.write(case['text'].encode('latin-1'))
    for order in ve.ORDERS:
        rec = case[order]
        want = (rec['out'], rec['ret'], rec['exc'])
        got = _run(lambda: magot_variants.heterozygosity_from_vcf(
            path, case['loci'], case['window'], order=order), capfd)
        assert got == want
        note = rec['note']
        if note in ('native', 'raise'):
            assert (rec['exc'] == 'KeyError') == (note == 'raise')
            assert magot_variants.heterozygosity_from_vcf.last_path == \
                ('heterozygosity_from_vcf', 'native', None)
        else:
            assert magot_variants.heterozygosity_from_vcf.last_path == \
                ('heterozygosity_from_vcf', 'host', note)
        got = _run(lambda: magot_variants.heterozygosity_from_vcf(
            path, case['loci'], case['window'], order=order, native='False'), capfd)
        assert got == want
    note = case['py2']['note']
    if note in engine._lib.VCF_REASONS:
        assert engine.VariantHets.parse(case['text'].encode('latin-1')) == (None, note)


def test_the_worlds_through_the_tool_equal_the_model(tmp_path, capfd):
    """the whole native path, the renderer and the orders included, where the
    loci are many and a contig is counted in pieces"""
    for n_data, n_samples in ((257, 33), (4099, 3)):
        text, loci = ve.world(n_data, n_samples)
        path = str(tmp_path / ('w%d.vcf' % n_data))
        with open(path, 'wb') as fh:
            fh.write(text.encode('latin-1'))
        for order in ve.ORDERS:
            for use in (loci, None):
                window = 97
                want = ve.expected(text, use, window, order)
                got = _run(lambda: magot_variants.heterozygosity_from_vcf(
                    path, use, window, order=order), capfd)
                assert got == want
                note = ve.native_note(text, use, window, order)
                assert magot_variants.heterozygosity_from_vcf.last_path[1:] == \
                    (('native', None) if note == 'native' else ('host', note))


# ---------------------------------------------------------------------------
# limits, timing, the command line
# ---------------------------------------------------------------------------

def test_the_limits_decline_with_their_reasons():
    text, loci = ve.world(65, 3)
    data = text.encode('latin-1')
    assert engine.VariantHets.parse(data, max_bytes=len(data) - 1) == (None, 'too_large')
    assert engine.VariantHets.parse(data, max_samples=2) == (None, 'too_many_samples')
    assert engine.VariantHets.parse(data, max_runs=3) == (None, 'too_many_runs')
    hets = _native(text, max_bytes=len(data), max_samples=3, max_runs=4)
    try:
        t = ve.table(text, loci, 'py2')
        hets.resolve([0] * hets.n_runs)
        split, samples, runs, counters = engine.VariantHets.params()
        # declined before anything of that size is allocated or read
        foreign, reason = ctypes.c_uint32(), ctypes.c_uint32()
        rc = engine._lib.lib().magot_vcf_count(hets.ctx.handle, hets.handle, None, None, None,
                                               counters // 3 + 1, None, None,
                                               ctypes.byref(foreign), ctypes.byref(reason))
        assert rc == engine._lib.ERR_UNSUPPORTED
        assert engine._lib.VCF_REASONS[reason.value] == 'too_many_counts'
        assert len(t['runs']) == hets.n_runs
    finally:
        hets.close()
    wide = ve.vcf([ve.row('c1', 5, *['0/1:%d' % s for s in range(samples + 1)])],
                  names=['n%d' % s for s in range(samples + 1)])
    assert engine.VariantHets.parse(wide.encode('latin-1')) == (None, 'too_many_samples')
    assert engine.VariantHets.parse(b'') == (None, 'no_header')
    assert engine.VariantHets.parse(ve.vcf([], names=()).encode('latin-1') +
                                    b'c1\t5\t.\tA\tC\t5\tPASS\t.\tGT\n') == (None, 'no_samples')


def test_the_most_samples_go_native():
    samples = engine.VariantHets.params()[1]
    rows = [ve.row('c1', 5 + k, *['%s:%d' % (('0/1', '1/1', '0|1')[(s + k) % 3], s % 50)
                                  for s in range(samples)]) for k in range(3)]
    text = ve.vcf(rows, names=['n%d' % s for s in range(samples)])
    hets = _native(text)
    try:
        assert hets.n_samples == samples
        _assert_equals_table(hets, text, ['c1,1,6', 'c1,100'], 'insertion')
    finally:
        hets.close()


def test_time_names_every_pass_and_the_answers_stand():
    text, loci = ve.world(4099, 3)
    hets = _native(text)
    try:
        _assert_equals_table(hets, text, loci, 'py2')
        t = hets.time(1)
        assert set(t) == set(engine.VariantHets.PASSES) | {'text_bytes'}
        assert t['text_bytes'] == len(text)
        assert all(t[k] > 0 for k in engine.VariantHets.PASSES)
        _assert_equals_table(hets, text, loci, 'insertion')
    finally:
        hets.close()


def test_the_command_line_in_a_process_of_its_own(tmp_path):
    case = GOLD['random_0']
    path = str(tmp_path / 'calls.vcf')
    with open(path, 'wb') as fh:
        fh.write(case['text'].encode('latin-1'))
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get('PYTHONPATH', ''),
               MAGOT_CLI_TIMING='0')
    res = subprocess.run([sys.executable, '-m', 'magot_amd.genome_tools', 'heterozygosity_from_vcf',
                          path, 'window=%d' % case['window']],
                         stdout=subprocess.PIPE, stderr=subprocess.PIPE, env=env, timeout=300)
    assert res.returncode == 0, res.stderr[-2000:]
    want = case['py2']
    assert want['note'] == 'native'
    assert res.stdout.decode('latin-1') == want['out'] + want['ret'] + '\n'
    assert genome_tools.TOOLS['heterozygosity_from_vcf'] is genome_tools.heterozygosity_from_vcf
