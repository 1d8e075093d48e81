"""write_gff's text on the device (gffwrite.hip): engine.GffWriter against
gffwrite_expect.render_rows, byte for byte, on row tables made here -- row
counts around the rows one wave renders and over several workgroups, output
lines and source columns at every misalignment, empty and long columns, names
longer than any staging bound, a last line without LF, one source line behind
four rows, integers of every width and sign, every score class and every
decline, the phases, references that leave the blob -- and convert_gff's native
path against the reference's goldens, its recorded runs and the object path.
The shapes derive from GffWriter.params()."""

import contextlib
import io
import os
import random

import pytest

import goldlib
import gffwrite_expect as gx
from magot_amd import engine, genome_tools
from magot_amd._lib import MagotError

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, 'tests', 'golden')
GOLD = gx.load()
CASES = gx.cases()
PARAMS = engine.GffWriter.params()
G = PARAMS['rows_per_group']
WAVES = PARAMS['threads'] // 64
ORDERS = ('insertion', 'py2')


def line(seqid=b'c1', source=b'src', ftype=b'CDS', lo=b'1', hi=b'9', score=b'.', strand=b'+',
         phase=b'0', tags=b'ID=x', end=b'\n'):
    return b'\t'.join([seqid, source, ftype, lo, hi, score, strand, phase, tags]) + end


class Table(object):
    """a text, a blob and rows over them"""

    def __init__(self):
        self.text, self.blob, self.items = b'', b'', []
        self.names = []  # (place in the blob, bytes), resolved once the text is whole

    def add_line(self, ln):
        off = len(self.text)
        self.text += ln
        return off

    def name(self, data):
        self.names.append((len(self.blob), data))
        self.blob += data
        return len(self.names) - 1

    def row(self, line_off, ident, parent=None, kind=gx.LINE, lo=1, hi=9, type_name=None):
        self.items.append((line_off, ident, parent, kind, lo, hi, type_name))

    def rows(self):
        n = len(self.text)
        items = []
        for line_off, ident, parent, kind, lo, hi, type_name in self.items:
            it = {'line_off': line_off, 'lo': lo, 'hi': hi, 'kind': kind,
                  'id_off': n + self.names[ident][0], 'id_len': len(self.names[ident][1])}
            if parent is not None:
                it['kind'] |= gx.HAS_PARENT
                it['parent_off'] = n + self.names[parent][0]
                it['parent_len'] = len(self.names[parent][1])
            if type_name is not None:
                it['type_off'] = n + self.names[type_name][0]
                it['type_len'] = len(self.names[type_name][1])
            items.append(it)
        return gx.make_rows(items)


def _render(text, blob, rows):
    w = engine.GffWriter.parse(text, blob, rows)
    assert isinstance(w, engine.GffWriter), w
    try:
        assert w.n_rows == len(rows)
        out = w.render().tobytes()
        assert w.out_bytes == len(out)
        return out
    finally:
        w.close()


def _assert_rendered(text, blob, rows):
    want = gx.render_rows(text, blob, rows)
    assert want is not None
    got = _render(text, blob, rows)
    assert got == want
    return got


def _seeded_table(n_rows, seed):
    rnd = random.Random(seed)
    t = Table()
    kinds = (gx.LINE, gx.EXON_TWIN, gx.GTF, gx.MADE_PARENT)
    tname = t.name(b'transcript')
    for k in range(n_rows):
        off = t.add_line(line(seqid=b'chr%d' % rnd.randrange(30), source=rnd.choice([b'a', b'srcX', b'']),
                              score=rnd.choice([b'.', b'1', b'0.50', b'-3', b'12.125', b'']),
                              strand=rnd.choice([b'+', b'-', b'.']),
                              phase=rnd.choice([b'0', b'1', b'2', b'.']),
                              tags=b'ID=n%d;Parent=p%d' % (k, k // 3)))
        kind = rnd.choice(kinds)
        ident = t.name(b'n%d' % k * rnd.randint(1, 3))
        parent = t.name(b'p%d' % (k // 3)) if (kind == gx.GTF or rnd.random() < 0.7) else None
        t.row(off, ident, parent, kind, rnd.randrange(10 ** rnd.randint(1, 9)),
              rnd.randrange(10 ** rnd.randint(1, 9)), tname if kind == gx.MADE_PARENT else None)
    return t


@pytest.mark.parametrize('n_rows', [0, 1, G - 1, G, G + 1, 5 * G + 3])
def test_row_counts_around_a_group(n_rows):
    t = _seeded_table(n_rows, 100 + n_rows)
    got = _assert_rendered(t.text, t.blob, t.rows())
    assert got.count(b'\n') == n_rows


def test_several_workgroups():
    n_rows = 9 * G * WAVES + 5
    t = _seeded_table(n_rows, 7)
    got = _assert_rendered(t.text, t.blob, t.rows())
    assert G * WAVES * 2 * 20 < len(got) < (1 << 20)


def test_output_lines_start_at_every_offset_mod_16():
    t = Table()
    seen = set()
    total = 0
    for k in range(3 * G):
        ident = t.name(b'i' * (k % 17 + 1))
        off = t.add_line(line())
        t.row(off, ident)
        seen.add(total % 16)
        total += len(gx.render_rows(t.text, t.blob, t.rows()[-1:]))
    assert seen == set(range(16))
    _assert_rendered(t.text, t.blob, t.rows())


def test_source_columns_start_at_every_misalignment():
    t = Table()
    ident = t.name(b'id')
    for pad in range(16):
        t.add_line(b'#' * pad + b'\n')
        for seqid in range(1, 17):
            off = t.add_line(line(seqid=b's' * seqid, source=b'q' * (pad + 1), score=b'0.25',
                                  strand=b'-'))
            t.row(off, ident)
    rows = t.rows()
    assert {int(o) % 16 for o in rows['line_off']} == set(range(16))
    _assert_rendered(t.text, t.blob, rows)


def test_empty_and_long_columns_and_names():
    t = Table()
    long_id = t.name(bytes(random.Random(3).choices(b'abcdefghij0123456789', k=4096)))
    parent = t.name(b'P' * 700)
    tname = t.name(b'T' * 300)
    a = t.add_line(line(seqid=b'', source=b''))
    b = t.add_line(line(seqid=b'S' * 300, source=b'R' * 129, strand=b'', phase=b''))
    # column 9 of 4 KiB lies behind the eighth tab: the size pass never walks it
    c = t.add_line(line(tags=b'ID=' + b'z' * 4096))
    for off in (a, b, c):
        for kind in (gx.LINE, gx.EXON_TWIN, gx.GTF, gx.MADE_PARENT):
            t.row(off, long_id, parent, kind, type_name=tname if kind == gx.MADE_PARENT else None)
            t.row(off, long_id, None if kind != gx.GTF else parent, kind,
                  type_name=tname if kind == gx.MADE_PARENT else None)
    got = _assert_rendered(t.text, t.blob, t.rows())
    assert got.startswith(b'\t\tCDS\t1\t9\t.\t+\t0\tID=')


def test_names_in_the_text_and_across_its_end():
    t = Table()
    off = t.add_line(line(tags=b'ID=abc;Parent=defg', end=b''))  # no LF behind the last line
    t.blob = b'XYZ'
    n = len(t.text)
    rows = gx.make_rows([
        {'line_off': off, 'lo': 5, 'hi': 6, 'kind': gx.LINE | gx.HAS_PARENT,
         'id_off': t.text.index(b'abc'), 'id_len': 3,
         'parent_off': t.text.index(b'defg'), 'parent_len': 4},
        {'line_off': off, 'lo': 5, 'hi': 6, 'kind': gx.LINE | gx.HAS_PARENT,
         'id_off': n - 2, 'id_len': 5, 'parent_off': n + 3, 'parent_len': 0}])
    got = _assert_rendered(t.text, t.blob, rows)
    assert got.endswith(b'ID=fgXYZ;Parent=\n')


def test_one_source_line_behind_four_rows():
    t = Table()
    gene, tx, cds = t.name(b'gA'), t.name(b'tA'), t.name(b'tA-CDS')
    tn, gn = t.name(b'transcript'), t.name(b'gene')
    off = t.add_line(line(score=b'7', tags=b'gene_id "gA"; transcript_id "tA";', end=b''))
    t.row(off, gene, None, gx.MADE_PARENT, 10, 50, gn)
    t.row(off, tx, gene, gx.MADE_PARENT, 10, 50, tn)
    t.row(off, cds, tx, gx.EXON_TWIN, 10, 50)
    t.row(off, cds, tx, gx.LINE, 10, 50)
    got = _assert_rendered(t.text, t.blob, t.rows())
    assert got == (b'c1\t.\tgene\t10\t50\t.\t+\t.\tID=gA\n'
                   b'c1\t.\ttranscript\t10\t50\t.\t+\t.\tID=tA;Parent=gA\n'
                   b'c1\tsrc\texon\t10\t50\t7.0\t+\t0\tID=ExonOftA-CDS;Parent=tA\n'
                   b'c1\tsrc\tCDS\t10\t50\t7.0\t+\t0\tID=tA-CDS;Parent=tA\n')


def test_integers_of_every_width_and_sign():
    t = Table()
    ident = t.name(b'i')
    off = t.add_line(line())
    values = [0, -1, -(2 ** 63), 2 ** 63 - 1]
    for width in range(1, 19):
        values += [10 ** (width - 1), 10 ** width - 1, -(10 ** (width - 1)), int('123456789' * 2)
                   % 10 ** width]
    for k, v in enumerate(values):
        t.row(off, ident, lo=v, hi=values[-1 - k])
    got = _assert_rendered(t.text, t.blob, t.rows())
    assert b'\t-9223372036854775808\t' in got and b'\t999999999999999999\t' in got


SCORES_A = [b'.', b'', b'-', b'+', b'-.', b'%', b' ', b'..']
SCORES_B = [b'1', b'0.50', b'-0', b'007', b'.5', b'-.5', b'1.', b'123456789012', b'-12.3400',
            b'0.0001', b'0.000123456789012', b'12345678.9012', b'000000000000000001',
            b'0.0000000', b'-000.000', b'100000000000', b'1.00000000000000000000', b'0', b'00.10']


def test_every_score_class_and_phase():
    t = Table()
    ident = t.name(b'i')
    for score in SCORES_A + SCORES_B:
        for phase in (b'0', b'1', b'2', b'.', b'3', b'', b'00'):
            t.row(t.add_line(line(score=score, phase=phase)), ident)
    rows = t.rows()
    got = _assert_rendered(t.text, t.blob, rows).split(b'\n')
    assert got[0].split(b'\t')[5:8] == [b'.', b'+', b'0']
    by_score = {s: got[7 * k].split(b'\t')[5] for k, s in enumerate(SCORES_A + SCORES_B)}
    assert all(by_score[s] == b'.' for s in SCORES_A)
    assert by_score[b'-0'] == b'-0.0' and by_score[b'007'] == b'7.0'
    assert by_score[b'0.0000000'] == b'0.0' and by_score[b'-000.000'] == b'-0.0'
    assert by_score[b'000000000000000001'] == b'1.0'
    for s in SCORES_B:
        assert by_score[s].decode() == '%s' % gx.py2_float_str(float(s)), s


@pytest.mark.parametrize('score', gx.SCORE_DECLINES)
def test_score_declines_raise_the_status(score):
    t = Table()
    ident = t.name(b'i')
    for k in range(G + 2):
        t.row(t.add_line(line(score=b'1' if k != G else score.encode())), ident)
    assert gx.render_rows(t.text, t.blob, t.rows()) is None
    got = engine.GffWriter.parse(t.text, t.blob, t.rows())
    assert got == (None, 'score', G + 1)


def test_a_made_parent_ignores_its_lines_score():
    t = Table()
    ident, tn = t.name(b'i'), t.name(b'gene')
    t.row(t.add_line(line(score=b'1e9', phase=b'2')), ident, None, gx.MADE_PARENT, type_name=tn)
    assert _assert_rendered(t.text, t.blob, t.rows()) == b'c1\t.\tgene\t1\t9\t.\t+\t.\tID=i\n'


def test_a_line_without_eight_tabs_declines():
    t = Table()
    ident = t.name(b'i')
    t.row(t.add_line(line()), ident)
    t.row(t.add_line(b'c1\tsrc\tCDS\t1\t9\t.\t+\n'), ident)
    t.add_line(line())
    assert engine.GffWriter.parse(t.text, t.blob, t.rows()) == (None, 'columns', 2)


@pytest.mark.parametrize('field', ['id', 'parent', 'type', 'line'])
def test_a_reference_past_the_blob_is_a_range_error(field):
    t = Table()
    ident, parent, tn = t.name(b'id'), t.name(b'par'), t.name(b'gene')
    off = t.add_line(line())
    t.row(off, ident, parent, gx.MADE_PARENT, type_name=tn)
    rows = t.rows()
    whole = len(t.text) + len(t.blob)
    _assert_rendered(t.text, t.blob, rows)
    if field == 'line':
        rows[0]['line_off'] = len(t.text) + 1
    else:
        rows[0][field + '_off'] = whole - int(rows[0][field + '_len']) + 1
    with pytest.raises(MagotError) as err:
        engine.GffWriter.parse(t.text, t.blob, rows)
    assert 'leaves the text and the blob' in str(err.value)


def _tool(path, input_format, output_format, order, native):
    buf = io.BytesIO()
    out = io.TextIOWrapper(buf, encoding='latin-1', newline='\n')
    with contextlib.redirect_stdout(out):
        genome_tools.convert_gff(path, input_format, output_format, order=order, native=native)
        out.flush()
    return buf.getvalue(), genome_tools.convert_gff.last_path


@pytest.mark.parametrize('cmd,want', gx.CKSUMS, ids=[' '.join(c[0]) for c in gx.CKSUMS])
def test_native_path_gives_the_reference_cksums(cmd, want):
    got, path = _tool(os.path.join(GOLDEN, cmd[0]), cmd[1], cmd[2], 'py2', 'True')
    assert path == ('convert_gff', 'native', None)
    assert goldlib.posix_cksum(got) == want


@pytest.mark.parametrize('name', sorted(CASES))
def test_recorded_cases_native_equals_object_path(name, tmp_path):
    p = tmp_path / 'in.gff'
    p.write_bytes(CASES[name]['gff'].encode('latin-1'))
    for fmt in sorted(gx.FORMATS):
        run = GOLD['cases'][name]['runs'][fmt]
        note = gx.path_note(CASES[name], fmt)
        for order in ORDERS:
            if run['exc']:
                with pytest.raises(Exception) as err:
                    _tool(str(p), 'gff3', fmt, order, 'True')
                assert type(err.value).__name__ == run['exc']
                continue
            got, path = _tool(str(p), 'gff3', fmt, order, 'True')
            assert path == ('convert_gff',) + (('native', None) if note == 'native'
                                               else ('host', note)), (fmt, order)
            assert got == _tool(str(p), 'gff3', fmt, order, 'False')[0], (fmt, order)
            if order == 'insertion':
                assert got == run['out'].encode('latin-1'), fmt


def test_ncbi_fixture_raises_through_the_native_call():
    """its ncRNAs keep no children once exons are ignored: the planner declines
    and the object path raises what the reference raises"""
    path = os.path.join(GOLDEN, 'O.biroi_NCBIrefseq_gff3Subset.gff')
    for fmt in sorted(gx.FORMATS):
        with pytest.raises(TypeError):
            _tool(path, 'gff3', fmt, 'py2', 'True')
        assert genome_tools.convert_gff.last_path == \
            ('convert_gff', 'host', 'write_gff takes a diagnostic path')
