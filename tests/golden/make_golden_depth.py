"""Record what the REFERENCE's own depth_from_gff prints: tests/golden/depth_from_gff.json.

Runs only where the reference is installed (see make_golden.py, whose
lib2to3 copy this imports); the reference function (genome_tools.py:598-652)
runs unchanged, and nothing of its program text is stored: only inputs,
outputs, hashes, exception names and the reason the native path must give
when it leaves a run to the host loop.

The copy runs under Python 3, which differs from the Python 2 target in three
places this function touches.  Files are opened with universal newlines and
``split()`` knows more separators: every input here is ASCII, free of
0x1c-0x1f, and ends its lines with '\\n' or '\\r\\n'.  Dicts iterate in
insertion order: each run is recorded twice, ``insertion`` as it runs, and
``py2`` with the *result* of the reference's read_gff wrapped at run time so
that every table is re-inserted in the CPython 2.7 order model's order
(oracle.magot_oracle.py2_order_after_deepcopy) -- the carry-over of a missing
contig and the "first CDS" then follow Python 2 -- and the printed CDS block
permuted by py2_dict_order of its parents afterwards.  A set's order is
hash-seeded under Python 3: the lines after '#missing from depth file' are
stored sorted (``missing``), apart from the rest (``head``), and compared as a
set.

Per case: ``depth`` (text) or ``depth_spec`` (depth_expect.spec_table) with
``depth_sha``; ``gff`` (text) or ``gff_file``; ``file_decline``: [reason,
line] engine.DepthTrack.parse must give, or null when it must take the table;
and ``runs``, each with ``features``, ``stream_length`` and per order
  exc      exception name, or null
  head, missing   the stdout (see above), or ``sha`` / ``len`` of head when long
  decline  why the native path must decline, or null when it must not (set
           here from the case's definition: part of the contract the tests
           check, not a reference output)

Usage:  python tests/golden/make_golden_depth.py
"""

import json
import os
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))

import make_golden  # noqa: E402
from make_golden import mo, sha  # noqa: E402
import depth_expect as de  # noqa: E402

KEEP_TEXT = 4096
DEFAULT = "['CDS','intron','upstream','downstream']"
BASE_SPEC = {'contigs': [['c1', 100], ['c2', 45]], 'mul': 7, 'mod': 13}
FIRST_CDS = 'the first CDS is on a contig missing from the depth file'
FIRST_TX = 'the first transcript is on a contig missing from the depth file'
STRAND = "a transcript strand other than '+' / '-'"


def base_lines():
    return de.spec_table(BASE_SPEC)[0].decode('latin-1').splitlines(True)


def edit(fn):
    lines = base_lines()
    fn(lines)
    return ''.join(lines)


def _swap(ls, i, j):
    ls[i], ls[j] = ls[j], ls[i]


EXAMPLE = [('t1', 'c1', '+', [(11, 30), (41, 60)]), ('t2', 'c2', '-', [(5, 20), (25, 40)]),
           ('t3', 'c3', '+', [(3, 9)])]
EXAMPLE_RUNS = [(DEFAULT, '1000'), (DEFAULT, '10'), (DEFAULT, '0'), (DEFAULT, '+5'),
                ("['CDS']", '10'), ("['upstream']", '10'), ("['intron','downstream']", '10'),
                ('[]', '10'), ("('upstream','CDS')", '7')]


def cases():
    """name -> (depth text, gff text, file_decline, [(features, stream_length, decline)]);
    decline None: native; a str: that reason; a callable (features list, exc)
    -> reason or None."""
    base = ''.join(base_lines())
    ex = de.gff_text(EXAMPLE)
    plain = [(DEFAULT, '10', None)]
    c = {}
    c['example'] = (base, ex, None, [(f, s, None) for f, s in EXAMPLE_RUNS])
    c['stream_length_bad'] = (base, ex, None, [
        (DEFAULT, '-5', 'stream_length < 0: a negative slice bound'),
        ("['CDS']", '-5', 'stream_length < 0: a negative slice bound'),
        (DEFAULT, 'abc', 'stream_length is not an integer'),
        (DEFAULT, '1.5', 'stream_length is not an integer')])
    c['features_bad'] = (base, ex, None, [
        ("'CDS upstream'", '10', 'features is not a container of strings'),
        ('5', '10', 'features is not a container of strings'),
        ("['CDS', 5]", '10', 'features is not a container of strings'),
        ('CDS', '10', 'features is not a literal')])  # a NameError, there and here
    c['minus_flank_past_end'] = (base, de.gff_text([('t1', 'c2', '-', [(30, 40)]),
                                                    ('t2', 'c2', '-', [(41, 45)]),
                                                    ('t3', 'c2', '-', [(40, 60)]),
                                                    ('t4', 'c1', '+', [(95, 130)])]), None, plain)
    c['plus_at_position_1'] = (base, de.gff_text([('t1', 'c1', '+', [(1, 10)]),
                                                  ('t2', 'c1', '+', [(3, 10)])]), None,
                               plain + [(DEFAULT, '1', None)])
    c['missing_middle'] = (base, de.gff_text([('t1', 'c1', '+', [(5, 9), (20, 29)]),
                                              ('t2', 'zz', '-', [(5, 9), (12, 15)]),
                                              ('t3', 'c2', '+', [(12, 15)])]), None,
                           [(DEFAULT, '10', first_missing), ("['upstream']", '10', first_missing)])
    many = [('m%d' % k, ['c1', 'gone%d' % (k % 3), 'c2', 'lost'][k % 4], '+-'[k % 2],
             [(3 + k, 9 + k), (20 + k, 24 + k)]) for k in range(12)]
    c['missing_many'] = (base, de.gff_text(many), None,
                         [(DEFAULT, '10', first_missing), ("['CDS']", '4', first_missing),
                          ("['upstream']", '4', first_missing)])
    c['missing_first'] = (base, de.gff_text([('t1', 'zz', '+', [(5, 9)]), ('t2', 'c1', '+', [(5, 9)])]),
                          None, [(DEFAULT, '10', first_missing), ("['upstream']", '10', first_missing)])
    c['missing_all'] = (base, de.gff_text([('t1', 'zz', '+', [(5, 9)]), ('t2', 'yy', '-', [(5, 9)])]),
                        None, [(DEFAULT, '10', FIRST_CDS), ("['upstream']", '10', FIRST_TX)])
    dot = de.gff_text([('t1', 'c1', '+', [(15, 19)]), ('t2', 'c1', '.', [(25, 29)]),
                       ('t3', 'c2', '?', [(5, 9)])])
    c['strand_dot'] = (base, dot, None, [(DEFAULT, '10', STRAND), ("['CDS']", '10', None),
                                         ("['upstream']", '10', STRAND)])
    c['strand_dot_first'] = (base, de.gff_text([('t1', 'c1', '.', [(15, 19)])]), None,
                             [(DEFAULT, '10', STRAND)])
    neg = 'a CDS start < 1 or end < 0: a negative slice bound'
    c['start_zero'] = (base, de.gff_text([('t1', 'c1', '+', [(0, 9), (20, 24)])]), None,
                       [(DEFAULT, '10', neg), ("['upstream']", '10',
                                               'a transcript start < 1 or end < 0: a negative slice bound')])
    c['start_negative'] = (base, de.gff_text([('t1', 'c1', '-', [(-5, 9)]), ('t2', 'c2', '+', [(2, 3)])]),
                           None, [(DEFAULT, '10', neg)])
    c['no_cds'] = (base, 'c1\tsrc\tmRNA\t5\t50\t.\t+\t.\tID=t1\n', None,
                   [(DEFAULT, '10', 'no CDS'), ("['CDS']", '10', 'no CDS')])
    c['transcript_without_cds'] = (
        base, de.gff_text([('t1', 'c1', '+', [(15, 19)])]) + 'c1\tsrc\tmRNA\t5\t50\t.\t+\t.\tID=t0\n',
        None, [(DEFAULT, '10', 'a transcript without coordinates'), ("['CDS']", '10', None)])
    c['cds_under_gene'] = (
        base, 'c1\tsrc\tgene\t5\t50\t.\t-\t.\tID=g1\nc1\tsrc\tCDS\t5\t20\t.\t-\t0\tID=x1;Parent=g1\n'
        'c1\tsrc\tCDS\t30\t50\t.\t-\t0\tID=x2;Parent=g1\n', None, plain)
    c['crlf_gff'] = (base, ex.replace('\n', '\r\n'), None, plain)

    # tables inside the native grammar
    c['table_crlf'] = (base.replace('\n', '\r\n'), ex, None, plain)
    c['table_spaces_columns'] = (
        ''.join(ln.replace('\t', ' \t  ', 1).replace('\n', '\tx  y \n') for ln in base_lines()),
        ex, None, plain)
    c['table_no_final_lf'] = (base[:-1], ex, None, plain)
    c['table_leading_zeros'] = (edit(lambda ls: ls.__setitem__(4, 'c1\t0005\t00000012\n')), ex, None,
                                plain)
    c['table_prefix_names'] = (
        de.table_text([('c1', de.formula_depths(30, 7, 13)), ('c10', de.formula_depths(20, 5, 11)),
                       ('c1x', de.formula_depths(25, 3, 17))]).decode('latin-1'),
        de.gff_text([('t1', 'c1', '+', [(11, 20)]), ('t2', 'c10', '-', [(5, 12)]),
                     ('t3', 'c1x', '+', [(13, 25)])]), None, plain)
    c['table_big_depths'] = (edit(lambda ls: (ls.__setitem__(14, 'c1\t15\t2147483647\n'),
                                              ls.__setitem__(15, 'c1\t16\t2147483647\n'),
                                              ls.__setitem__(16, 'c1\t17\t0\n'))), ex, None, plain)

    # tables outside it: the reason and the first offending line
    def bad(name, fn, reason, line):
        text = edit(fn)
        c[name] = (text, ex, [reason, line], [(DEFAULT, '10', 'depth file: %s at line %d' % (reason, line))])

    bad('bad_empty_line', lambda ls: ls.insert(50, '\n'), 'empty line', 51)
    bad('bad_empty_line_first', lambda ls: ls.insert(0, '\n'), 'empty line', 1)
    bad('bad_crlf_only_line', lambda ls: ls.insert(7, '\r\n'), 'empty line', 8)
    bad('bad_two_fields', lambda ls: ls.__setitem__(119, 'c2\t20\n'), 'fewer than three fields', 120)
    bad('bad_one_field', lambda ls: ls.append('c2\n'), 'fewer than three fields', 146)
    bad('bad_leading_blank', lambda ls: ls.__setitem__(10, ' c1\t11\t5\n'), 'leading blank', 11)
    bad('bad_sign_position', lambda ls: ls.__setitem__(10, 'c1\t+11\t5\n'), 'sign on a number', 11)
    bad('bad_sign_depth', lambda ls: ls.__setitem__(144, 'c2\t45\t-3\n'), 'sign on a number', 145)
    bad('bad_vertical_tab', lambda ls: ls.__setitem__(3, 'c1\x0b4\t5\n'), 'byte outside the grammar', 4)
    bad('bad_form_feed_column', lambda ls: ls.__setitem__(3, 'c1\t4\t5\tx\x0cy\n'),
        'byte outside the grammar', 4)
    bad('bad_depth_float', lambda ls: ls.__setitem__(20, 'c1\t21\t3.5\n'), 'not a number', 21)
    bad('bad_position_word', lambda ls: ls.__setitem__(20, 'c1\tx21\t3\n'), 'not a number', 21)
    bad('bad_eleven_digits', lambda ls: ls.__setitem__(30, 'c1\t31\t12345678901\n'),
        'number out of range', 31)
    bad('bad_above_int32', lambda ls: ls.__setitem__(0, 'c1\t1\t2147483648\n'), 'number out of range', 1)
    bad('bad_long_name', lambda ls: ls.append('N' * 256 + '\t1\t4\n'), 'name longer than 255 bytes', 146)
    bad('bad_swapped_positions', lambda ls: _swap(ls, 40, 41), 'position out of sequence', 41)
    bad('bad_skipped_position', lambda ls: ls.pop(49), 'position out of sequence', 50)
    bad('bad_duplicate_position', lambda ls: ls.insert(60, 'c1\t60\t999\n'), 'position out of sequence', 61)
    bad('bad_position_zero', lambda ls: ls.insert(100, 'c1\t0\t9\n'), 'position out of sequence', 101)
    bad('bad_run_from_two', lambda ls: ls.pop(100), 'position out of sequence', 101)
    bad('bad_position_past_count', lambda ls: ls.__setitem__(144, 'c2\t4500\t3\n'),
        'position out of sequence', 145)
    bad('bad_repeated_contig', lambda ls: ls.extend('c1\t%d\t%d\n' % (p, p % 5) for p in range(1, 31)),
        'repeated contig', 146)
    bad('bad_interleaved', lambda ls: ls.insert(120, 'c1\t101\t7\n'), 'position out of sequence', 121)
    return c


def first_missing(features, exc):
    if exc != 'UnboundLocalError':
        return None
    return FIRST_CDS if 'CDS' in features else FIRST_TX


def py2_tables(read_gff):
    """read_gff whose result's tables iterate in Python 2's order"""
    def wrapped(*args, **kwargs):
        aset = read_gff(*args, **kwargs)
        if aset is not None:
            for name, table in list(aset.__dict__.items()):
                if type(table) is dict:
                    aset.__dict__[name] = {k: table[k] for k in mo.py2_order_after_deepcopy(list(table))}
        return aset
    return wrapped


def permute_cds_block(out):
    """the lines after '#CDS counts' in py2_dict_order of their parents"""
    lines = out.splitlines(True)
    if not lines or lines[0] != '#CDS counts\n':
        return out
    n = 1
    while n < len(lines) and not lines[n].startswith('#'):
        n += 1
    block = {ln.split('\t')[0]: ln for ln in lines[1:n]}
    assert len(block) == n - 1
    return ''.join(lines[:1] + [block[p] for p in mo.py2_dict_order(list(block))] + lines[n:])


def record(out, exc, keep):
    head, missing = de.split_missing(out)
    e = {'exc': exc, 'missing': sorted(missing)}
    if len(head) <= keep:
        e['head'] = head
    else:
        e['sha'], e['len'] = sha(head), len(head)
    return e


def run_both(ref, tools, depth_path, gff_path, features, stream_length, decline, keep=KEEP_TEXT):
    entry = {'features': features, 'stream_length': stream_length}
    plain_read = ref.read_gff
    for order in ('insertion', 'py2'):
        ref.read_gff = py2_tables(plain_read) if order == 'py2' else plain_read
        try:
            _, exc, out = make_golden.call(lambda: tools.depth_from_gff(
                depth_path, gff_path, features=features, stream_length=stream_length))
        finally:
            ref.read_gff = plain_read
        if order == 'py2':
            out = permute_cds_block(out)
        entry[order] = record(out, exc, keep)
        why = decline
        if callable(decline):
            try:
                flist = eval(features, {}, {})  # the generator's own literals
            except Exception:  # noqa: BLE001
                flist = []
            why = decline(flist, exc)
        entry[order]['decline'] = why
    return entry


def main():
    ref = make_golden.reference_module()
    import genome_tools as tools
    out = {}
    with tempfile.TemporaryDirectory() as tmp:
        dp, gp = os.path.join(tmp, 'depth.txt'), os.path.join(tmp, 'in.gff')
        for name, (depth, gff, file_decline, runs) in cases().items():
            assert all(ord(ch) < 128 and not 0x1c <= ord(ch) <= 0x1f for ch in depth + gff)
            assert '\r' not in (depth + gff).replace('\r\n', '')
            for path, text in ((dp, depth), (gp, gff)):
                with open(path, 'w', encoding='latin-1', newline='') as fh:
                    fh.write(text)
            out[name] = {'depth': depth, 'gff': gff, 'file_decline': file_decline,
                         'runs': [run_both(ref, tools, dp, gp, f, s, why) for f, s, why in runs]}
            print(name, [(r['insertion']['exc'], r['py2']['exc']) for r in out[name]['runs']],
                  flush=True)
        spec = de.obiroi_spec()
        text, _ = de.spec_table(spec)
        with open(dp, 'wb') as fh:
            fh.write(text)
        out['obiroi'] = {'depth_spec': spec, 'depth_sha': sha(text), 'gff_file': de.OBIROI_GFF,
                         'file_decline': None,
                         'runs': [run_both(ref, tools, dp, os.path.join(HERE, de.OBIROI_GFF),
                                           DEFAULT, '1000', None, keep=0)]}
        print('obiroi', [out['obiroi']['runs'][0][o].get('sha', '')[:8] for o in ('insertion', 'py2')],
              flush=True)
    with open(os.path.join(HERE, 'depth_from_gff.json'), 'w') as fh:
        json.dump({'cases': out}, fh, indent=0, sort_keys=True)
        fh.write('\n')


if __name__ == '__main__':
    main()
