"""convert_gff without a device: genome.write_gff / get_gff (the object path)
against the reference's three goldens, its recorded runs and the field model of
gffwrite_expect.py; the host planner's rows (magot_gff_lower_write) rendered by
gffwrite_expect.render_rows against the same; the score rule against Python 2's
str(float); the row struct against the header."""

import io
import contextlib
import os
import random
import re
import subprocess
import sys

import pytest

import goldlib
import gffwrite_expect as gx
from magot_amd import _lib, engine, genome, genome_tools, py2order

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, 'tests', 'golden')
GOLD = gx.load()
CASES = gx.cases()
NAMES = sorted(CASES)
ORDERS = ('insertion', 'py2')


def _object_path(path, input_format, output_format, order):
    buf = io.StringIO()
    with contextlib.redirect_stdout(buf):
        genome_tools.convert_gff(path, input_format, output_format, order=order, native='False')
    return buf.getvalue().encode('latin-1')


def _lowered(data, fmt, order):
    """(rows, blob) of the planner, or None where it declines"""
    read = engine.GffRead.read(data, for_write=True)
    if read is None:
        return None
    try:
        plan = read.lower_write(gx.FORMATS[fmt], order)
        if plan is None:
            return None
        return plan.rows.copy(), bytes(plan.blob)
    finally:
        read.close()


def _planner_text(data, fmt, order):
    low = _lowered(data, fmt, order)
    if low is None:
        return None
    body = gx.render_rows(data, low[1], low[0])
    return None if body is None else (body[:-1] + b'\n')


@pytest.fixture(scope='module')
def case_files(tmp_path_factory):
    d = tmp_path_factory.mktemp('gffwrite')
    out = {}
    for name, case in CASES.items():
        p = d / (name + '.gff')
        p.write_bytes(case['gff'].encode('latin-1'))
        out[name] = str(p)
    return out


def test_golden_file_is_current():
    assert sorted(GOLD['cases']) == NAMES
    for name in NAMES:
        assert GOLD['cases'][name]['gff'] == CASES[name]['gff'], name
        assert GOLD['cases'][name]['path'] == CASES[name]['path'], name
    assert [tuple(c[0]) for c in GOLD['cksums']] == [c[0] for c in gx.CKSUMS]


@pytest.mark.parametrize('cmd,want', gx.CKSUMS, ids=[' '.join(c[0]) for c in gx.CKSUMS])
def test_object_path_gives_the_reference_cksums(cmd, want):
    got = _object_path(os.path.join(GOLDEN, cmd[0]), cmd[1], cmd[2], 'py2')
    assert goldlib.posix_cksum(got) == want


@pytest.mark.parametrize('cmd,want', gx.CKSUMS, ids=[' '.join(c[0]) for c in gx.CKSUMS])
def test_cli_in_a_fresh_process_gives_the_reference_cksums(cmd, want):
    env = dict(os.environ, PYTHONPATH=ROOT)
    got = subprocess.run([sys.executable, '-m', 'magot_amd.genome_tools', 'convert_gff',
                          cmd[0], cmd[1], cmd[2], 'native=False'], cwd=GOLDEN, env=env,
                         stdout=subprocess.PIPE, check=True).stdout
    assert goldlib.posix_cksum(got) == want


@pytest.mark.parametrize('cmd,want', gx.CKSUMS, ids=[' '.join(c[0]) for c in gx.CKSUMS])
def test_planner_rows_give_the_reference_cksums(cmd, want):
    with open(os.path.join(GOLDEN, cmd[0]), 'rb') as fh:
        data = fh.read()
    got = _planner_text(data, cmd[2], 'py2')
    assert got is not None
    assert goldlib.posix_cksum(got) == want


@pytest.mark.parametrize('name', NAMES)
@pytest.mark.parametrize('fmt', sorted(gx.FORMATS))
def test_recorded_case_on_the_object_path(name, fmt, case_files):
    run = GOLD['cases'][name]['runs'][fmt]
    if run['exc']:
        with pytest.raises(Exception) as err:
            _object_path(case_files[name], 'gff3', fmt, 'insertion')
        assert type(err.value).__name__ == run['exc']
    else:
        assert _object_path(case_files[name], 'gff3', fmt, 'insertion') == \
            run['out'].encode('latin-1')


@pytest.mark.parametrize('name', NAMES)
@pytest.mark.parametrize('fmt', sorted(gx.FORMATS))
def test_recorded_case_through_the_planner(name, fmt):
    """the planner lowers what its path note says, to the reference's bytes,
    and to the object path's in Python 2 order"""
    case = CASES[name]
    data = case['gff'].encode('latin-1')
    note = gx.path_note(case, fmt)
    run = GOLD['cases'][name]['runs'][fmt]
    got = _planner_text(data, fmt, 'insertion')
    if note == 'native':
        assert got == run['out'].encode('latin-1')
        aset = genome.read_gff(case['gff'])
        want = (genome.write_gff(aset, gx.FORMATS[fmt], 'py2') + '\n').encode('latin-1')
        assert _planner_text(data, fmt, 'py2') == want
    else:
        assert got is None
    if run['exc']:
        assert note != 'native'


def test_unknown_output_format_prints_the_message(case_files):
    got = _object_path(case_files['gff3_two_genes'], 'gff3', 'bed', 'py2')
    assert got == b"currently only writes 'gff3' and 'gtf' format\n"


def test_extended_gff3_and_augustus_hint():
    aset = genome.read_gff(CASES['shadowing_attribute']['gff'])
    z = aset['z']
    assert z.get_gff('extended gff3') == \
        'c1\ts\tCDS\t130\t140\t9\t+\t0\tID=z;Parent=t1;parent=t1'
    assert z.get_gff('augustus hint CDSpart M') == 'c1\ts\tCDSpart\t130\t140\t9\t+\t0\tsrc=M'
    assert z.get_gff('augustus hint CDSpart M 4') == \
        'c1\ts\tCDSpart\t130\t140\t9\t+\t0\tsrc=M;pri=4'
    t = aset['t1'].get_gff('augustus hint exonpart E')
    assert t.split('\n') == ['c1\tsrc\texonpart\t10\t50\t.\t+\t0\tsrc=E',
                             'c1\tsrc\texonpart\t80\t120\t.\t+\t1\tsrc=E',
                             'c1\ts\texonpart\t130\t140\t9\t+\t0\tsrc=E']
    with pytest.raises(UnboundLocalError):
        z.get_gff('bed')
    assert aset['g1'].get_gff('extended gff3').split('\n')[1] == \
        'c1\tsrc\tmRNA\t10\t140\t.\t+\t.\tID=t1;Parent=g1;parent=g1'
    with pytest.raises(TypeError):  # ';gene_id ' + None
        genome.read_gff(CASES['gene_id_only_gtf']['gff'])['gA-CDS'].get_gff('gtf')


def test_float_scores_print_as_python_2_does():
    aset = genome.read_gff(CASES['gff3_scores']['gff'])
    cols = [aset['C%d' % k].get_gff().split('\t')[5] for k in range(12)]
    assert cols == ['1.0', '0.5', '-0.0', '.', '.', '.', '7.0', '0.5', '123456789012.0',
                    '-12.34', '0.0001', '1.0']
    assert genome_tools._py2_float_str is py2order.py2_float_str


def test_sibling_clashes_follow_the_clash_key():
    aset = genome.read_gff(CASES['sibling_clash']['gff'])
    ids = [re.search('ID=([a-z])', ln).group(1)
           for ln in aset['t'].get_gff().split('\n')[1:]]
    # a (10,50); b (10,51); c: clash -> (10,52); d: (10,52) taken -> (10,55);
    # e: -> (10,54); f: -> (10,55) replaces d
    assert ids == ['a', 'b', 'c', 'e', 'f']
    aset = genome.read_gff(CASES['clash_overwrites']['gff'])
    ids = [re.search('ID=([a-z])', ln).group(1)
           for ln in aset['t'].get_gff().split('\n')[1:]]
    assert ids == ['a', 'c']  # c's clash key (10, 52) replaces b


def test_exon_added_moves_cds_lines_behind_at_every_level():
    aset = genome.read_gff(CASES['identical_cds_lines']['gff'])
    lines = aset['g'].get_gff('exon added gff3').split('\n')
    kinds = [ln.split('\t')[2] for ln in lines]
    assert kinds == ['gene', 'mRNA'] + ['exon'] * 4 + ['mRNA', 'exon'] + ['CDS'] * 5
    assert [re.search('ID=([^;]*)', ln).group(1) for ln in lines[-5:]] == \
        ['x', 'x2', 'x-3', 'x-4', 'y']


@pytest.mark.parametrize('name,fmt', [('shadowing_attribute', 'gff3'), ('cr_in_a_column', 'gff3'),
                                      ('source_named_cds', 'exon_added_gff3'),
                                      ('parent_holds_id_equals', 'exon_added_gff3')])
def test_planner_declines(name, fmt):
    data = CASES[name]['gff'].encode('latin-1')
    for order in ORDERS:
        assert _lowered(data, fmt, order) is None


def test_renamed_ids_and_crlf_names_come_from_the_blob():
    data = CASES['identical_cds_lines']['gff'].encode('latin-1')
    rows, blob = _lowered(data, 'gff3', 'insertion')
    assert blob.startswith(b'x2x-3x-4gene')  # the made-up IDs, then the tables' names
    assert sorted(int(o) - len(data) for o in rows['id_off'] if o >= len(data)) == [0, 2, 5]
    data = CASES['crlf_line_ends']['gff'].encode('latin-1')
    rows, blob = _lowered(data, 'gff3', 'insertion')
    assert b'\r' not in blob and blob  # the CR-stripped copies of column 9's last name


@pytest.mark.parametrize('order', ORDERS)
@pytest.mark.parametrize('fmt', ['gff3', 'exon_added_gff3'])
def test_two_top_level_tables_follow_the_dict_model(order, fmt):
    """regions beside genes: which table comes first under Python 2 is the
    expect module's own dict's answer, not py2order's"""
    case = CASES['regions_and_genes_whole']
    aset = genome.read_gff(case['gff'])
    want = gx.write_model(gx.model_of(aset), gx.FORMATS[fmt], order)
    assert want.count('\tregion\t') == 2 and want.count('\tgene\t') == 2
    assert genome.write_gff(aset, gx.FORMATS[fmt], order) == want
    assert _planner_text(case['gff'].encode('latin-1'), fmt, order) == (want + '\n').encode()


def test_attribute_name_order_is_the_models():
    names = ['gene', 'transcript', 'CDS', 'UTR', 'genome', 'region', 'mRNA', 'chromosome',
             'match', 'match_part', 'similarity', 'ncRNA', 'tRNA', 'rRNA', 'exon2']
    for n in range(1, len(names) + 1):
        for copies in (0, 1, 2):
            assert py2order.names_after_copies(names[:n], copies) == \
                gx.py2_names(names[:n], copies)


def test_ncbi_fixture_raises_on_both_paths():
    path = os.path.join(GOLDEN, 'O.biroi_NCBIrefseq_gff3Subset.gff')
    with pytest.raises(TypeError):
        _object_path(path, 'gff3', 'gff3', 'py2')
    with open(path, 'rb') as fh:
        data = fh.read()
    for fmt in gx.FORMATS:
        assert _lowered(data, fmt, 'py2') is None


def _digit_strings(longest):
    out = ['']
    for width in range(1, longest + 1):
        out += ['%0*d' % (width, v) for v in range(10 ** width)]
    return out


def _check_literal(lit):
    got = gx.score_text(lit)
    assert got is not None, lit
    assert got == py2order.py2_float_str(float(lit)), lit


def test_score_rule_agrees_with_python_2():
    """The expect module's rule on literals of the three forms with up to 4
    integer and 4 fraction digits: every integer part beside every fraction of
    up to 2 digits, every fraction beside every integer part of up to 1 digit,
    100000 seeded draws from the whole product, and 3000 seeded literals of up
    to 12 significant digits.  The whole product, 2.5e8 literals, is walked in
    compiled code by tests/test_sanitize_gffwrite.py, which also holds that
    program's rule against this one."""
    whole4, whole1 = _digit_strings(4), _digit_strings(1)
    frac4, frac2 = _digit_strings(4), _digit_strings(2)
    seen = 0
    for wholes, fracs in ((whole4, frac2), (whole1, frac4)):
        for w in wholes:
            if w:
                _check_literal(w)          # -?D+
                _check_literal('-' + w)
            for f in fracs:
                if w or f:
                    _check_literal(w + '.' + f)  # -?D+.D* and -?.D+
                    seen += 1
    assert seen > 1300000
    rnd = random.Random(20261021)
    for _ in range(100000):
        w, f = rnd.choice(whole4), rnd.choice(frac4)
        if w or f:
            _check_literal(rnd.choice(('', '-')) + w + '.' + f)
    for _ in range(3000):
        digits = ''.join(rnd.choice('0123456789') for _ in range(rnd.randint(1, 12)))
        cut = rnd.randint(0, len(digits))
        lit = rnd.choice(['', '-']) + digits[:cut] + '.' + digits[cut:]
        got = gx.score_text(lit)
        if got is not None:  # 0.0000x and the like decline
            assert got == py2order.py2_float_str(float(lit)), lit
    for lit in ('.', '', '-', '+', '%', '-.', ' '):
        assert gx.score_text(lit) == '.'
        with pytest.raises(ValueError):
            float(lit)
    for lit in gx.SCORE_DECLINES:
        assert gx.score_text(lit) is None, lit


def test_row_struct_size_is_the_headers():
    with open(os.path.join(ROOT, 'include', 'magot.h')) as fh:
        body = re.search(r'typedef struct magot_gffrow \{(.*?)\} magot_gffrow;', fh.read(),
                         re.S).group(1)
    body = re.sub(r'/\*.*?\*/', '', body, flags=re.S)
    size = {'uint64_t': 8, 'int64_t': 8, 'uint32_t': 4}
    total, names = 0, []
    for decl in body.split(';'):
        decl = decl.strip()
        if decl:
            kind, fields = decl.split(None, 1)
            for f in fields.split(','):
                total += size[kind]
                names.append(f.strip())
    assert total == 64 == gx.ROW_DTYPE.itemsize == _lib.GFFROW_DTYPE.itemsize
    assert tuple(names) == gx.ROW_DTYPE.names == _lib.GFFROW_DTYPE.names
    assert [gx.ROW_DTYPE.fields[n][1] for n in names] == \
        [_lib.GFFROW_DTYPE.fields[n][1] for n in names]
