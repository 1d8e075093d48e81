"""Record what the REFERENCE's own position_dic does: tests/golden/position_dic.json.

Runs only where the reference is installed (see make_golden.py, whose
lib2to3 copy this imports); the reference class (genome.py:981-1100) runs
unchanged, and nothing of its program text is stored: only inputs, outputs,
hashes and exception names.

The copy runs under Python 3, where ``range(len(...) / window_jump)``
(genome.py:1048) would divide to a float.  ``window_jump`` is therefore passed
as an ``int`` subclass whose ``__rtruediv__`` floor-divides: Python 2's integer
division there, an ordinary int everywhere else.

Per case (tests/track_expect.py runs them, here against the reference and in
the tests against magot_amd.genome):
  genome, dtype   the position_dic's genome (``genomes``, or the shipped
                  O.biroi subset) and dtype
  setup           producer steps applied first (verbose off)
  call            the recorded step: at_content, fill, count or sliding
  exc             exception name, or null
  stdout          the captured prints (sha256 + length when long)
  result          the return value (lists over a few hundred entries as
                  sha256 + length; regions as [ID, seqid, coords, type])
  arrays          every array afterwards (bool: hex of the packed bits, or
                  their sha256 above 4096 bases)
  decline         why the device path must leave this call to the host, or
                  null when it must take it (set here from the case's
                  definition: part of the contract the tests check, not a
                  reference output)

Usage:  python tests/golden/make_golden_positions.py
"""

import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))

import make_golden  # noqa: E402
import track_expect as te  # noqa: E402


class Py2Jump(int):
    """An int that floor-divides when something is divided by it."""

    def __rtruediv__(self, other):
        return other // int(self)


TOY = [['c1', 'ATATGCGCatatNNNNATTTTAAAGGGCCCATATATATAT'], ['c2', 'AT'],
       ['c3', 'GGGGCCCCATATATATATGGGGCCCCAAAATTTTNNacgt']]
GENOMES = {
    'toy': TOY,
    'shorter': [['c1', TOY[0][1][:25]], TOY[1], TOY[2]],
    'missing': [TOY[0], TOY[1]],
    'extra': TOY + [['c4', 'ttttACGTNNNN']],
}
AT = [{'op': 'at_content', 'genome': 'toy'}]
AT_OB = [{'op': 'at_content', 'genome': 'obiroi'}]
HOST_ONLY = 'fill_from_annotations runs on the host'


def ann(*features):
    return {'feature': 'CDS', 'features': [list(f) for f in features]}


INSIDE = ann(('f1', 'c1', 3, 10), ('f2', 'c3', 38, 40), ('f3', 'c1', 8, 12), ('f4', 'c2', 1, 2),
             ('f5', 'c3', 1, 40), ('f6', 'c1', 7, 7))


def sliding(name, decline=None, dtype='bool', setup=AT, genome='toy', verbose=False, **kw):
    return {'name': name, 'genome': genome, 'dtype': dtype, 'setup': setup,
            'call': {'op': 'sliding', 'kw': kw, 'verbose': verbose}, 'decline': decline}


def cases():
    c = []
    for op in ('sum', 'average'):
        for w, j in ((5, 1), (5, 2), (5, 3), (1, 1), (32, 1), (39, 1), (40, 1), (41, 1), (5, 41),
                     (5, 35), (2, 7)):
            c.append(sliding('dict_%s_w%d_j%d' % (op, w, j), window_size=w, window_jump=j,
                             operation=op))
    c.append(sliding('dict_defaults', window_size=4))
    for j in (1, 2, 3):
        c.append(sliding('regions_average_0.8_j%d' % j, window_size=5, window_jump=j,
                         operation='average', output='annotation_set', threshold=0.8))
        c.append(sliding('regions_sum_3_j%d' % j, window_size=5, window_jump=j, operation='sum',
                         output='annotation_set', threshold=3))
    for thr in (0, 6, 5, 1, 2.5):
        c.append(sliding('regions_sum_thr%s' % thr, window_size=5, window_jump=1, operation='sum',
                         output='annotation_set', threshold=thr))
    for thr in (0.0, 1.0, 1.01, 0.6, 0.2):
        c.append(sliding('regions_average_thr%s' % thr, window_size=5, window_jump=2,
                         operation='average', output='annotation_set', threshold=thr))
    c.append(sliding('regions_default_threshold', window_size=3, output='annotation_set'))
    c.append(sliding('exclude_c1_dict', window_size=5, seqs_to_exclude=['c1']))
    c.append(sliding('exclude_c1_regions', window_size=5, window_jump=2, operation='average',
                     output='annotation_set', threshold=0.8, seqs_to_exclude=['c1']))
    c.append(sliding('exclude_all', window_size=5, seqs_to_exclude=['c1', 'c3', 'c2']))
    c.append(sliding('verbose_dict', verbose=True, window_size=5, window_jump=2))
    c.append(sliding('verbose_regions', verbose=True, window_size=5, window_jump=2,
                     operation='average', output='annotation_set', threshold=0.8))
    c.append(sliding('verbose_regions_sum_j1', verbose=True, window_size=4, window_jump=1,
                     output='annotation_set', threshold=3))
    c.append(sliding('coords_below', 'output "coords"', window_size=5, output='coords',
                     threshold=[100, 200]))
    c.append(sliding('coords_at', 'output "coords"', window_size=5, output='coords',
                     threshold=[0, 10]))
    c.append(sliding('set_dict', 'operation "set"', window_size=5, window_jump=3,
                     operation='set'))
    c.append(sliding('set_regions', 'operation "set"', window_size=5, operation='set',
                     output='annotation_set'))
    c.append(sliding('int_dtype_dict', 'an int track', dtype='int', window_size=5, window_jump=2))
    c.append(sliding('int_dtype_regions', 'an int track', dtype='int', window_size=5,
                     window_jump=2, operation='average', output='annotation_set', threshold=0.8))
    fives = [{'op': 'fill', 'ann': INSIDE, 'fill_type': 'coords', 'fill_with': '5'}]
    c.append(sliding('int_dtype_fives', 'an int track', dtype='int', setup=fives, window_size=5,
                     window_jump=1))
    c.append(sliding('empty_track', setup=[], window_size=5, output='annotation_set'))

    for dtype in ('bool', 'int'):
        for ft in ('coords', 'start'):
            for fw in ('1', '0', 'True', '5'):
                c.append({'name': 'fill_%s_%s_%s' % (dtype, ft, fw), 'genome': 'toy',
                          'dtype': dtype, 'setup': AT,
                          'call': {'op': 'fill', 'ann': INSIDE, 'fill_type': ft, 'fill_with': fw},
                          'decline': HOST_ONLY})
    odd = {'wrap': ann(('w', 'c1', 0, 3)), 'past_end': ann(('a', 'c3', 2, 4), ('p', 'c1', 38, 45)),
           'unknown_seqid': ann(('a', 'c3', 2, 4), ('k', 'nope', 1, 3), ('b', 'c1', 1, 2)),
           'empty_range': ann(('e', 'c1', 9, 3), ('e2', 'nope', 5, 4))}
    for nm, a in odd.items():
        for ft in ('coords', 'start'):
            c.append({'name': 'fill_%s_%s' % (nm, ft), 'genome': 'toy', 'dtype': 'bool',
                      'setup': [], 'call': {'op': 'fill', 'ann': a, 'fill_type': ft,
                                            'fill_with': '1'}, 'decline': HOST_ONLY})
    c.append({'name': 'fill_unknown_type', 'genome': 'toy', 'dtype': 'bool', 'setup': [],
              'call': {'op': 'fill', 'ann': INSIDE, 'fill_type': 'stop', 'fill_with': '1'},
              'decline': HOST_ONLY})

    c.append({'name': 'count_inside', 'genome': 'toy', 'dtype': 'bool', 'setup': AT,
              'call': {'op': 'count', 'ann': INSIDE}, 'decline': None})
    c.append({'name': 'count_zero_track', 'genome': 'toy', 'dtype': 'bool', 'setup': [],
              'call': {'op': 'count', 'ann': INSIDE}, 'decline': None})
    c.append({'name': 'count_no_features', 'genome': 'toy', 'dtype': 'bool', 'setup': AT,
              'call': {'op': 'count', 'ann': ann()}, 'decline': None})
    c.append({'name': 'count_empty_range', 'genome': 'toy', 'dtype': 'bool', 'setup': AT,
              'call': {'op': 'count', 'ann': ann(('e', 'c1', 9, 3), ('f', 'c1', 2, 9))},
              'decline': None})
    why = {'wrap': 'a feature outside its contig', 'past_end': 'a feature outside its contig',
           'unknown_seqid': 'a feature on an unknown contig'}
    for nm in why:
        c.append({'name': 'count_' + nm, 'genome': 'toy', 'dtype': 'bool', 'setup': AT,
                  'call': {'op': 'count', 'ann': odd[nm]}, 'decline': why[nm]})
    c.append({'name': 'count_int_fives', 'genome': 'toy', 'dtype': 'int', 'setup': AT + [
        {'op': 'fill', 'ann': ann(('x', 'c1', 5, 9)), 'fill_type': 'coords', 'fill_with': '5'}],
        'call': {'op': 'count', 'ann': INSIDE}, 'decline': 'an int track'})

    c.append({'name': 'at_content', 'genome': 'toy', 'dtype': 'bool', 'setup': [],
              'call': {'op': 'at_content', 'genome': 'toy'}, 'decline': None})
    c.append({'name': 'at_content_over_bits', 'genome': 'toy', 'dtype': 'bool',
              'setup': [{'op': 'fill', 'ann': INSIDE, 'fill_type': 'start', 'fill_with': '1'}],
              'call': {'op': 'at_content', 'genome': 'toy'}, 'decline': None})
    c.append({'name': 'at_content_int', 'genome': 'toy', 'dtype': 'int', 'setup': [],
              'call': {'op': 'at_content', 'genome': 'toy'}, 'decline': 'an int track'})
    c.append({'name': 'at_content_extra_contig', 'genome': 'toy', 'dtype': 'bool', 'setup': [],
              'call': {'op': 'at_content', 'genome': 'extra'}, 'decline': None})
    c.append({'name': 'at_content_shorter_contig', 'genome': 'toy', 'dtype': 'bool', 'setup': [],
              'call': {'op': 'at_content', 'genome': 'shorter'},
              'decline': 'a contig of another length'})
    c.append({'name': 'at_content_missing_contig', 'genome': 'toy', 'dtype': 'bool', 'setup': [],
              'call': {'op': 'at_content', 'genome': 'missing'}, 'decline': 'a missing contig'})
    c.append({'name': 'at_content_longer_contig', 'genome': 'shorter', 'dtype': 'bool',
              'setup': [], 'call': {'op': 'at_content', 'genome': 'toy'},
              'decline': 'a contig of another length'})

    ob = {'feature': 'CDS', 'gff_file': te.OBIROI_GFF}
    c.append({'name': 'obiroi_at_content', 'genome': 'obiroi', 'dtype': 'bool', 'setup': [],
              'call': {'op': 'at_content', 'genome': 'obiroi'}, 'decline': None})
    c.append(sliding('obiroi_sum', genome='obiroi', setup=AT_OB, window_size=10000,
                     window_jump=1000))
    c.append(sliding('obiroi_average', genome='obiroi', setup=AT_OB, window_size=10000,
                     window_jump=1000, operation='average'))
    c.append(sliding('obiroi_regions', genome='obiroi', setup=AT_OB, window_size=10000,
                     window_jump=1000, operation='average', output='annotation_set',
                     threshold=0.62))
    c.append(sliding('obiroi_regions_verbose', genome='obiroi', setup=AT_OB, verbose=True,
                     window_size=10000, window_jump=1000, operation='average',
                     output='annotation_set', threshold=0.62))
    c.append({'name': 'obiroi_fill_cds', 'genome': 'obiroi', 'dtype': 'bool', 'setup': [],
              'call': {'op': 'fill', 'ann': ob, 'fill_type': 'coords', 'fill_with': '1'},
              'decline': HOST_ONLY})
    # some genes there have only ncRNA children without base features: their
    # get_coords() raises TypeError
    c.append({'name': 'obiroi_count_gene', 'genome': 'obiroi', 'dtype': 'bool', 'setup': AT_OB,
              'call': {'op': 'count', 'ann': dict(ob, feature='gene')},
              'decline': 'a feature whose coordinates raise'})
    for ft in ('mRNA', 'CDS'):
        c.append({'name': 'obiroi_count_' + ft, 'genome': 'obiroi', 'dtype': 'bool',
                  'setup': AT_OB, 'call': {'op': 'count', 'ann': dict(ob, feature=ft)},
                  'decline': None})
    c.append(sliding('obiroi_cds_density', genome='obiroi', window_size=2000, window_jump=500,
                     output='annotation_set', threshold=1000,
                     setup=[{'op': 'fill', 'ann': ob, 'fill_type': 'coords', 'fill_with': '1'}]))
    return c


def main():
    ref = make_golden.reference_module()
    cache = {}
    out = []
    for case in cases():
        pd, res, exc, so = te.run_case(ref, case, GENOMES, cache, jump_wrap=Py2Jump)
        rec = dict(case)
        rec.update(te.outcome(pd, res, exc, so))
        out.append(rec)
        print(case['name'], exc, len(so), flush=True)
    assert len({r['name'] for r in out}) == len(out)
    with open(os.path.join(HERE, 'position_dic.json'), 'w') as fh:
        json.dump({'genomes': GENOMES, 'cases': out}, fh, indent=0, sort_keys=True)
        fh.write('\n')


if __name__ == '__main__':
    main()
