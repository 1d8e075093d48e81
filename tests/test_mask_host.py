"""mask_from_gff on the host (genome_tools.py:394-428): the forced line loop
of magot_amd.genome_tools.mask_from_gff against every run recorded from the
reference in tests/golden/mask_from_gff.json (stdout, exceptions, both contig
orders), and the native planner (engine.MaskPlan / engine.mask_fasta_check)
against the same file: it declines exactly the runs marked ``decline`` and
its interval table reproduces every other run's output."""

import numpy as np
import pytest

import mask_expect as me
from magot_amd import _lib, engine, genome_tools

CASES = me.load_cases()
RUNS = me.all_runs(CASES)
VALID_OVERWRITE = ('True', 'T', 'true', 't', 'TRUE') + me.KEEP


def _ids(runs):
    return ['%s-%s' % (name, me.run_id(CASES[name]['runs'][i])) for name, i in runs]


def _loop(paths, run, order, capfdbinary):
    exc = None
    try:
        genome_tools.mask_from_gff(paths[0], paths[1], mask_type=run['mask_type'],
                                   overwrite_softmask=run['overwrite_softmask'],
                                   feature_type=run['feature_type'], order=order, native='False')
    except Exception as e:  # noqa: BLE001
        exc = type(e).__name__
    return capfdbinary.readouterr().out, exc


@pytest.mark.parametrize('name,i', RUNS, ids=_ids(RUNS))
def test_line_loop_equals_the_reference(name, i, tmp_path, capfdbinary):
    case = CASES[name]
    run = case['runs'][i]
    paths = me.case_files(case, tmp_path)
    out, exc = _loop(paths, run, 'insertion', capfdbinary)
    assert exc == run['exc']
    if 'text' in run:
        assert out.decode('latin-1') == run['text']
    assert me.sha(out) == run['sha']
    out2, exc2 = _loop(paths, run, 'py2', capfdbinary)
    assert exc2 == run['exc'] and me.sha(out2) == run['sha_py2']


def _native_inputs(case):
    """(fasta bytes, gff bytes, [(name, bytes)] or None) as the native path reads them."""
    fa, gf = me.case_inputs(case)
    contigs = engine.fasta_read(fa, truncate_names=True)
    if contigs is not None and not (contigs and engine.mask_fasta_check(fa, len(contigs))):
        contigs = None
    return fa, gf, contigs


PLAN_RUNS = [(n, i) for n, i in RUNS
             if CASES[n]['runs'][i]['mask_type'] in ('soft', 'hard')
             and CASES[n]['runs'][i]['overwrite_softmask'] in VALID_OVERWRITE]


@pytest.mark.parametrize('name,i', PLAN_RUNS, ids=_ids(PLAN_RUNS))
def test_planner_declines_or_reproduces_the_reference(name, i):
    case = CASES[name]
    run = case['runs'][i]
    hard, keep = run['mask_type'] == 'hard', run['overwrite_softmask'] in me.KEEP
    fa, gf, contigs = _native_inputs(case)
    plan = None
    if contigs is not None:
        plan = engine.MaskPlan.build(gf, [nm for nm, _ in contigs], [len(s) for _, s in contigs],
                                     feature_type=run['feature_type'], hard=hard, keep_case=keep)
    if run['decline'] is not None:
        assert plan is None, run['decline']
        return
    assert plan is not None, _lib.lib().magot_last_error()
    try:
        assert (plan.hard, plan.keep_case) == (hard, keep)
        assert int(plan.intervals['len'].max(initial=0)) <= plan.piece
        cov = me.coverage(plan.intervals, [len(s) for _, s in contigs])
    finally:
        plan.close()
    names = [nm for nm, _ in contigs]
    assert names == run['contigs']
    masked = [me.apply_mask(s, c, hard, keep) for (_, s), c in zip(contigs, cov)]
    text = me.text_of(names, masked)
    assert me.sha(text) == run['sha']
    if 'text' not in run:
        return
    assert text.decode('latin-1') == run['text']
    # the coverage the reference's output implies: wherever masking a base
    # shows (its masked byte differs from its unmasked one), it changed
    # exactly where the table covers it
    lines = run['text'].split('\n')[1::2]
    for (_, s), c, got in zip(contigs, cov, lines):
        plain = me.apply_mask(s, np.zeros(len(s), bool), hard, keep)
        shows = me.apply_mask(s, np.ones(len(s), bool), hard, keep) != plain
        changed = np.frombuffer(got.encode('latin-1'), np.uint8) != plain
        assert np.array_equal(changed[shows], c[shows]) and not changed[~shows].any()


def test_long_intervals_are_split_into_pieces():
    piece = int(_lib.lib().magot_mask_piece())
    assert piece == 2048
    n = 5 * piece + 77
    gff = 'c\ts\tCDS\t2\t%d\t.\t+\t.\tx\nc\ts\tCDS\t10\t11\t.\t+\t.\tx\n' % n
    plan = engine.MaskPlan.build(gff, ['c'], [n], feature_type='CDS')
    try:
        iv = plan.intervals
    finally:
        plan.close()
    assert iv['contig'].tolist() == [0] * 7
    assert iv['start'].tolist() == [1 + k * piece for k in range(6)] + [9]
    assert iv['len'].tolist() == [piece] * 5 + [76, 2]
    # the golden case: two long overlapping features, every piece within bounds
    case = CASES['long_interval']
    _, gf, contigs = _native_inputs(case)
    plan = engine.MaskPlan.build(gf, [nm for nm, _ in contigs], [len(s) for _, s in contigs])
    try:
        assert len(plan.intervals) > 3 and int(plan.intervals['len'].max()) == piece
    finally:
        plan.close()


def test_decline_reasons_are_all_covered_and_integers_follow_the_flank_planner():
    # every reason the planner may decline for has a golden case ...
    reasons = {r['decline'] for c in CASES.values() for r in c['runs'] if r['decline']}
    for part in ('unknown seqid', 'bad integer', 'start < 1', 'stop < 0', 'list grows',
                 "whitespace directly after '>'", 'an empty contig', 'a repeated name',
                 'sequence before the first header', 'reader returns None', 'invalid argument'):
        assert any(part in r for r in reasons), part
    # ... except integers the reference reads and magot_flank_plan does not
    # (19 digits and more), which no golden case can hold: the Python 3 copy
    # of the reference would loop over range() of them
    line = 'c\ts\tCDS\t%s\t%s\t.\t+\t.\tx\n'
    for a, b, ok in (('1', '5', True), (' +2 ', '\x0b4', True), ('1', '9' * 18, True),
                     ('1', '1' + '0' * 18, False), ('1_0', '20', False), ('0x1', '5', False),
                     ('1', '5L', False), ('', '5', False), ('-', '5', False)):
        plan = engine.MaskPlan.build(line % (a, b), ['c'], [50])
        assert (plan is not None) == ok, (a, b)
        if plan is not None:
            plan.close()


def test_cli_is_registered(tmp_path, capfdbinary):
    assert genome_tools.TOOLS['mask_from_gff'] is genome_tools.mask_from_gff
    case = CASES['basic']
    run = case['runs'][2]
    fa, gf = me.case_files(case, tmp_path)
    assert genome_tools.main(['mask_from_gff', fa, gf, 'mask_type=hard', 'native=False',
                              'order=insertion']) == 0
    assert capfdbinary.readouterr().out.decode('latin-1') == run['text']
    with pytest.raises(ValueError):
        genome_tools.mask_from_gff(fa, gf, order='sorted')
