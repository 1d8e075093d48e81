"""depth_from_gff's host loop (genome_tools.py:598-652 restated; CPU only)
against the reference's own output (tests/golden/depth_from_gff.json) in both
table orders, exception names included, and against depth_expect's numpy
restatement on seeded random cases."""

import numpy as np
import pytest

import depth_expect as de
from magot_amd import genome_tools, py2order

GOLD = de.load()
CASES = GOLD['cases']
RUNS = [(name, i) for name in sorted(CASES) for i in range(len(CASES[name]['runs']))]


def _loop(paths, features, stream_length, order, capfdbinary):
    exc = None
    try:
        genome_tools.depth_from_gff(paths[0], paths[1], features=features,
                                    stream_length=stream_length, order=order, native='False')
    except Exception as e:  # noqa: BLE001
        exc = type(e).__name__
    return capfdbinary.readouterr().out, exc


@pytest.mark.parametrize('name,i', RUNS, ids=['%s-%d' % r for r in RUNS])
def test_host_loop_equals_the_reference(name, i, tmp_path, capfdbinary):
    case = CASES[name]
    run = case['runs'][i]
    paths = de.case_files(case, tmp_path)
    for order in ('insertion', 'py2'):
        out, exc = _loop(paths, run['features'], run['stream_length'], order, capfdbinary)
        de.same_as_recorded(out, exc, run[order])
        assert genome_tools.depth_from_gff.last_path[:2] == ('depth_from_gff', 'host')


def test_host_loop_equals_the_restatement(tmp_path, capfdbinary):
    """200 seeded small cases: contigs the table lacks, CDS and flanks past
    the contig end, every features subset."""
    rng = np.random.default_rng(20261019)
    raised = 0
    for n in range(200):
        contigs, transcripts, features, stream_length = de.random_case(rng)
        paths = de.case_files({'depth': de.table_text(contigs).decode('latin-1'),
                               'gff': de.gff_text(transcripts)}, tmp_path)
        cds = [(t, k) for t, tx in enumerate(transcripts) for k in range(len(tx[3]))]
        cds_ids = ['%s.c%d' % (transcripts[t][0], k) for t, k in cds]
        tx_ids = [tx[0] for tx in transcripts]
        for order in ('insertion', 'py2'):
            if order == 'py2':
                cds_order = [cds[cds_ids.index(i)] for i in py2order.order_after_copies(cds_ids, 1)]
                tx_order = [tx_ids.index(i) for i in py2order.order_after_copies(tx_ids, 1)]
                reorder = py2order.dict_order
            else:
                cds_order, tx_order, reorder = cds, list(range(len(transcripts))), list
            want, want_exc = de.expected(contigs, transcripts, features, stream_length, cds_order,
                                         tx_order, reorder, reorder)
            out, exc = _loop(paths, repr(features), stream_length, order, capfdbinary)
            assert (out.decode('latin-1'), exc) == (want, want_exc), (n, order)
            raised += exc is not None
    assert 0 < raised < 200  # both outcomes are met


def test_tool_is_registered_and_documented(tmp_path, capfdbinary):
    assert genome_tools.TOOLS['depth_from_gff'] is genome_tools.depth_from_gff
    assert 'depth_from_gff' in genome_tools.__doc__
    case = CASES['example']
    run = case['runs'][1]
    dp, gp = de.case_files(case, tmp_path)
    assert genome_tools.main(['depth_from_gff', dp, gp, 'stream_length=10', 'native=False',
                              'order=insertion']) == 0
    de.same_as_recorded(capfdbinary.readouterr().out, None, run['insertion'])
    with pytest.raises(ValueError):
        genome_tools.depth_from_gff(dp, gp, order='sorted')
