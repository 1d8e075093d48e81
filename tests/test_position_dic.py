"""genome.position_dic on the host (``native=False``) against the reference's
own recorded results (tests/golden/position_dic.json), the numpy restatements
of track_expect against the same records, and at_content_from_fasta's line
loop.  No device is needed."""

import json
import os

import numpy as np
import pytest

import track_expect as te
from magot_amd import genome, genome_tools

GOLD = te.load()
CASES = {c['name']: c for c in GOLD['cases']}
CACHE = {}
RECORDED = ('stdout', 'stdout_sha', 'stdout_n', 'exc', 'result', 'arrays')


def recorded(case):
    return {k: case[k] for k in RECORDED if k in case}


def as_json(x):
    return json.loads(json.dumps(x))


def test_the_goldens_cover_what_they_must():
    assert len(CASES) == len(GOLD['cases']) > 100
    assert [len(s) for _, s in GOLD['genomes']['toy']] == [40, 2, 40]
    # the example of the merge quirk: one region over two separate runs
    assert CASES['regions_average_0.8_j2']['result']['regions'][0] == \
        ['c1-window1', 'c1', [1, 27], 'region']
    assert CASES['dict_sum_w40_j1']['result'] == {'dict': {}, 'keys': []}
    assert [len(v) for v in CASES['dict_sum_w39_j1']['result']['dict'].values()] == [1, 1]
    assert CASES['dict_sum_w5_j41']['result']['dict'] == {'c1': [], 'c3': []}
    assert CASES['coords_below']['result'] == {'list': []} and CASES['coords_at']['exc'] == 'NameError'
    assert CASES['fill_past_end_coords']['exc'] == 'IndexError'
    assert CASES['fill_unknown_seqid_coords']['exc'] == 'KeyError'
    assert CASES['at_content_shorter_contig']['exc'] == 'IndexError'
    assert CASES['at_content_missing_contig']['exc'] == 'KeyError'
    assert CASES['verbose_dict']['stdout'] and CASES['verbose_regions']['stdout']
    assert any(c['decline'] is None for c in GOLD['cases'])


@pytest.mark.parametrize('name', sorted(CASES))
def test_host_path_reproduces_the_reference(name):
    case = CASES[name]
    pd, res, exc, out = te.run_case(genome, case, GOLD['genomes'], CACHE, native=False)
    assert as_json(te.outcome(pd, res, exc, out)) == recorded(case)
    assert pd.last_path[1] == 'host'


def test_results_hold_python_numbers_and_a_deep_copy():
    g = te.genome_of(genome, GOLD['genomes'], 'toy', CACHE)
    pd = genome.position_dic(g)
    pd.at_content(g, native=False)
    was, genome.verbose = genome.verbose, False
    try:
        sums = pd.sliding_window_calculate(5, 2, native=False)
        avg = pd.sliding_window_calculate(5, 2, operation='average', native=False)
        regions = pd.sliding_window_calculate(5, 2, operation='average', output='annotation_set',
                                              threshold=0.8, native=False)
    finally:
        genome.verbose = was
    assert all(type(v) is int for v in sums['c1']) and all(type(v) is float for v in avg['c1'])
    assert isinstance(regions, genome.AnnotationSet)
    r = regions.region['c1-window1']
    assert isinstance(r, genome.BaseAnnotation) and r.coords == (1, 27)
    assert r.annotation_set is regions and r.feature_type == 'region'
    counts = pd.count_from_annotations(te.annotations_of(
        genome, {'feature': 'CDS', 'features': [['a', 'c1', 1, 8]]}, {}), 'CDS', native=False)
    assert counts == [['a', 4, 4]] and all(type(v) is int for v in counts[0][1:])


def toy_arrays():
    return {sid: te.base_class(seq.encode()) for sid, seq in GOLD['genomes']['toy']}


def test_restated_base_class_matches_the_reference():
    want = CASES['at_content']['arrays']
    for sid, arr in toy_arrays().items():
        assert np.array_equal(arr, te.decode_bits(want[sid])), sid
    assert not te.base_class(b'ATatNn-*RYkm').tolist()[4:].count(True)
    assert te.base_class(b'ACGTacgtN', gc=True).tolist() == [False, True, True, False] * 2 + [False]


SLIDING = [n for n, c in CASES.items() if c['call']['op'] == 'sliding' and c['genome'] == 'toy'
           and c['dtype'] == 'bool' and c['setup'] == [{'op': 'at_content', 'genome': 'toy'}]
           and c['exc'] is None and c['call']['kw'].get('operation', 'sum') != 'set'
           and c['call']['kw'].get('output', 'dict') in ('dict', 'annotation_set')]


@pytest.mark.parametrize('name', SLIDING)
def test_restated_windows_and_regions_match_the_reference(name):
    case = CASES[name]
    kw = case['call']['kw']
    w, j = kw['window_size'], kw.get('window_jump', 1)
    op, thr = kw.get('operation', 'sum'), kw.get('threshold', 1)
    skip = kw.get('seqs_to_exclude', [])
    got_dict, got_regions = {}, []
    for sid, arr in toy_arrays().items():
        if len(arr) <= w or sid in skip:
            continue
        sums = te.window_sums(arr, w, j)
        values = [int(s) if op == 'sum' else int(s) * 1.0 / w for s in sums]
        got_dict[sid] = values
        passes = [v >= thr for v in values]
        walk = te.regions_walk(passes, w, j, len(arr))
        assert te.regions_from_flips(te.flips_of(passes), w, j, len(arr)) == walk
        # the integer form of the test, as the device applies it
        s_min = genome._min_passing_sum(w, op, thr)
        assert [int(s) >= s_min for s in sums] == passes
        got_regions += [['%s-window%d' % (sid, c[0]), sid, c, 'region'] for c in walk]
    if kw.get('output', 'dict') == 'dict':
        assert case['result'] == {'dict': got_dict, 'keys': list(got_dict)}
    else:
        assert case['result'] == {'regions': got_regions}


def test_restated_counts_match_the_reference():
    arrays = toy_arrays()
    case = CASES['count_inside']
    want = [[ID] + te.counts(arrays[sid], first - 1, last)
            for ID, sid, first, last in case['call']['ann']['features']]
    assert case['result'] == {'list': want}


def test_min_passing_sum():
    f = genome._min_passing_sum
    assert f(5, 'sum', 3) == 3 and f(5, 'sum', 0) == 0 and f(5, 'sum', 6) == 6
    assert f(5, 'sum', 2.5) == 3 and f(5, 'sum', -1) == 0 and f(5, 'sum', float('nan')) == 6
    assert f(5, 'average', 0.8) == 4 and f(5, 'average', 1.0) == 5 and f(5, 'average', 1.01) == 6
    assert f(10000, 'average', 0.62) == 6200 and f(3, 'average', 1 / 3.0) == 1
    for w in (3, 7, 10, 49, 1000):
        for k in range(w + 1):
            assert f(w, 'average', k * 1.0 / w) == k


# -- at_content_from_fasta ----------------------------------------------------

def run_tool(path, capfdbinary, **kw):
    exc = None
    try:
        genome_tools.at_content_from_fasta(path, **kw)
    except Exception as e:  # noqa: BLE001
        exc = type(e).__name__
    return capfdbinary.readouterr().out, exc


def test_at_content_from_fasta_line_loop_on_obiroi(golden_dir, capfdbinary):
    path = os.path.join(golden_dir, te.OBIROI_FA)
    out, exc = run_tool(path, capfdbinary, native='False')
    assert exc is None
    with open(path, 'rb') as fh:
        data = fh.read()
    assert out == te.at_content_lines(data)
    rows = [ln.split(b'\t') for ln in out.splitlines()]
    assert len(rows) == 6
    # the same counts from the reference's recorded at_content arrays
    want = CASES['obiroi_at_content']['arrays']
    for name, ats, gcs in rows:
        sid = name.decode()
        ones = want[sid]['ones'] if 'ones' in want[sid] else int(te.decode_bits(want[sid]).sum())
        assert int(ats) == ones and 0 < int(ats) + int(gcs) <= want[sid]['n']


FALLBACK_FILES = {
    'gt_inside_a_line': (b'>a x\nACGT\nAC>GT\nTTTT\n', b'a x\t2\t2\nC>GT\t4\t0\n', None),
    'empty_record': (b'>a\n>b\nacgtn\n', b'a\t0\t0\nb\t2\t2\n', None),
    'repeated_name': (b'>a\nAT\n>a\nGGC\n', b'a\t2\t0\na\t0\t3\n', None),
    'crlf_and_blank_lines': (b'>a one\r\nACGTNN\r\n\n\r\nacgu\r\n>b\r\nGG', b'a one\t3\t4\nb\t0\t2\n',
                             None),
    'sequence_first': (b'ACGT\n>a\nAC\n', b'', 'UnboundLocalError'),
    'blank_then_header': (b'\n>a\nAC\n', b'a\t1\t1\n', None),
    'empty_file': (b'', b'', 'UnboundLocalError'),
}


@pytest.mark.parametrize('name', sorted(FALLBACK_FILES))
def test_at_content_from_fasta_line_loop(name, tmp_path, capfdbinary):
    data, want, want_exc = FALLBACK_FILES[name]
    path = str(tmp_path / 'in.fa')
    with open(path, 'wb') as fh:
        fh.write(data)
    out, exc = run_tool(path, capfdbinary, native='False')
    assert (out, exc) == (want, want_exc)
    if want_exc is None:
        assert out == te.at_content_lines(data)


def test_tool_is_listed():
    assert genome_tools.TOOLS['at_content_from_fasta'] is genome_tools.at_content_from_fasta
    assert 'at_content_from_fasta <fasta>' in genome_tools.__doc__
