"""What convert_gff / write_gff must print, restated for the tests.

Nothing here imports the code under test.  Four parts:

  * the score and phase rules of the device path (``score_text``,
    ``phase_text``): a score column prints '.', a normalised literal, or is
    outside the device path (None);
  * ``render_rows``: the bytes a table of output rows stands for (the layout of
    ``magot_gffrow`` in include/magot.h, declared here a second time);
  * the field model: ``model_of`` flattens an annotation set into plain dicts
    and ``write_model`` restates genome.py:228-238, 616-645 and 733-778 over
    them, with a CPython 2.7 dict of its own (``Py2Dict``) for ``order='py2'``;
  * ``cases()`` / ``load()``: the recorded reference runs
    (tests/golden/gffwrite.json, made by tests/golden/make_golden_gffwrite.py).
"""

import json
import os
import re

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, 'golden', 'gffwrite.json')

ROW_DTYPE = np.dtype([('line_off', '<u8'), ('lo', '<i8'), ('hi', '<i8'), ('id_off', '<u8'),
                      ('parent_off', '<u8'), ('type_off', '<u8'), ('id_len', '<u4'),
                      ('parent_len', '<u4'), ('type_len', '<u4'), ('kind', '<u4')])
LINE, EXON_TWIN, GTF, MADE_PARENT = 0, 1, 2, 3
HAS_PARENT = 0x100
FORMATS = {'gff3': 'simple gff3', 'gtf': 'gtf', 'exon_added_gff3': 'exon added gff3'}

# The reference's own goldens (test_data/test_suite.py:15-17): POSIX cksum, size
CKSUMS = (
    (('minimalGFF3.gff', 'gff3', 'gtf'), (1904390924, 226225)),
    (('StandardGTF.gtf', 'gtf', 'gff3'), (2934568300, 276674)),
    (('StandardGTF.gtf', 'gtf', 'exon_added_gff3'), (2624776569, 512324)),
)

# Score columns the device path must hand back (the issue's list; a bare '+' has neither
# digit nor letter, float() refuses it and it prints '.': class (a))
SCORE_DECLINES = ('1e5', '1E-3', '1234567890123', '0.1234567890123', '0.00001', 'inf', 'nan',
                  '-inf', ' 1', '1 ', '+1', '+.5', '1.2.3', '--1', '1-', 'abc', '0x10', '1_0',
                  '123456789012.5', '1000000000000', '-.00001', '0.000012')


def py2_float_str(value):
    text = '%.12g' % value
    return text if ('.' in text or 'e' in text or 'n' in text) else text + '.0'


_SCORE = re.compile(r'(-?)([0-9]*)(\.?)([0-9]*)\Z')


def score_text(field):
    """'.' (class a), the normalised literal (class b), or None (declined)."""
    if not re.search('[0-9A-Za-z]', field):
        return '.'
    m = _SCORE.match(field)
    if not m:
        return None
    sign, whole, dot, frac = m.groups()
    if not (whole or (dot and frac)):
        return None
    lead = len(frac) - len(frac.lstrip('0'))
    whole = whole.lstrip('0')
    frac = frac.rstrip('0')
    if whole:
        span = len(whole) + len(frac)
    else:
        span = len(frac) - lead if frac else 0
    if len(whole) > 12 or span > 12 or (not whole and frac and lead > 3):
        return None
    return sign + (whole or '0') + '.' + (frac or '0')


def phase_text(field):
    return field if field in ('0', '1', '2') else '.'


def _ref(text, blob, off, length):
    whole = bytes(text) + bytes(blob)
    assert off + length <= len(whole)
    return whole[off:off + length]


def render_rows(text, blob, rows):
    """The bytes of every row's line, each ended by LF; None when a score is
    outside the device path or a source line lacks its eight tabs."""
    text = bytes(text)
    out = []
    for r in rows:
        start = int(r['line_off'])
        end = text.find(b'\n', start)
        line = text[start:len(text) if end < 0 else end]
        cols = line.split(b'\t')
        if len(cols) < 9:
            return None
        kind, has_parent = int(r['kind']) & 0xff, bool(int(r['kind']) & HAS_PARENT)
        ident = _ref(text, blob, int(r['id_off']), int(r['id_len']))
        parent = _ref(text, blob, int(r['parent_off']), int(r['parent_len'])) if has_parent else b''
        if kind == MADE_PARENT:
            score, phase = '.', '.'
        else:
            score = score_text(cols[5].decode('latin-1'))
            phase = phase_text(cols[7].decode('latin-1'))
            if score is None:
                return None
        c2, c3 = cols[1], cols[2]
        if kind == MADE_PARENT:
            c2, c3 = b'.', _ref(text, blob, int(r['type_off']), int(r['type_len']))
        elif kind == EXON_TWIN:
            c3 = b'exon'
        if kind == GTF:
            tail = b'transcript_id ' + ident + b';gene_id ' + parent
        else:
            tail = (b'ID=ExonOf' if kind == EXON_TWIN else b'ID=') + ident
            if has_parent:
                tail += b';Parent=' + parent
        out.append(b'\t'.join([cols[0], c2, c3, b'%d' % int(r['lo']), b'%d' % int(r['hi']),
                               score.encode(), cols[6], phase.encode(), tail]) + b'\n')
    return b''.join(out)


def make_rows(items):
    """rows from dicts of the fields that differ from zero"""
    rows = np.zeros(len(items), ROW_DTYPE)
    for k, it in enumerate(items):
        for name, v in it.items():
            rows[k][name] = v
    return rows


# ---------------------------------------------------------------------------
# A CPython 2.7 dict of str keys (64-bit, no -R): only what iteration order needs
# ---------------------------------------------------------------------------

_M64 = (1 << 64) - 1


def _hash(key):
    if not key:
        return 0
    h = (ord(key[0]) << 7) & _M64
    for ch in key:
        h = ((h * 1000003) & _M64) ^ ord(ch)
    h ^= len(key)
    return _M64 - 1 if h == _M64 else h


class Py2Dict(object):
    def __init__(self):
        self.table = [None] * 8
        self.fill = 0

    def _slot(self, table, key):
        mask = len(table) - 1
        h = _hash(key)
        i, perturb = h & mask, h
        while table[i & mask] is not None and table[i & mask] != key:
            i = (5 * i + perturb + 1) & _M64
            perturb >>= 5
        return i & mask

    def _resize(self, minused):
        size = 8
        while size <= minused:
            size <<= 1
        old, self.table = self.table, [None] * size
        for k in old:
            if k is not None:
                self.table[self._slot(self.table, k)] = k

    def add(self, key):  # PyDict_SetItem
        i = self._slot(self.table, key)
        if self.table[i] is None:
            self.table[i] = key
            self.fill += 1
            if self.fill * 3 >= len(self.table) * 2:
                self._resize((2 if self.fill > 50000 else 4) * self.fill)

    def update_from(self, other):  # PyDict_Merge into this (empty) dict
        n = len(other.keys())
        if (self.fill + n) * 3 >= len(self.table) * 2:
            self._resize((self.fill + n) * 2)
        for k in other.keys():
            i = self._slot(self.table, k)
            if self.table[i] is None:
                self.table[i] = k
                self.fill += 1

    def keys(self):
        return [k for k in self.table if k is not None]


def py2_keys(keys, copies):
    """a table's keys after insertion and ``copies`` deepcopies"""
    for _ in range(copies + 1):
        d = Py2Dict()
        for k in keys:
            d.add(k)
        keys = d.keys()
    return keys


def py2_names(names, copies):
    """an old-style instance's attribute names after ``copies`` deepcopies:
    _deepcopy_dict re-inserts, then y.__dict__.update(state)"""
    d = Py2Dict()
    for k in names:
        d.add(k)
    for _ in range(copies):
        state = Py2Dict()
        for k in d.keys():
            state.add(k)
        d = Py2Dict()
        d.update_from(state)
    return d.keys()


# ---------------------------------------------------------------------------
# The field model
# ---------------------------------------------------------------------------

def model_of(aset):
    """{'names': attribute names as set, 'copies': n, 'tables': {name: {ID:
    feature}}}; a feature is a dict: base, ID, parent, children, coords (base),
    cols (seqid, source, type, score, strand, phase as printed, '.' when the
    attribute is missing)."""
    def col(obj, name):
        if not hasattr(obj, name):
            return '.'
        v = getattr(obj, name)
        return py2_float_str(v) if type(v) is float else str(v)

    held = aset.__dict__
    model = {'names': [n for n in held if n != '_magot_copies'],
             'copies': held.get('_magot_copies', 0), 'tables': {}}
    for name, table in held.items():
        if type(table) is not dict:
            continue
        out = model['tables'][name] = {}
        for key, obj in table.items():
            base = type(obj).__name__ == 'BaseAnnotation'
            out[key] = {'base': base, 'ID': obj.ID, 'parent': obj.parent,
                        'children': None if base else list(obj.child_list),
                        'coords': tuple(obj.coords) if base else None,
                        'cols': [col(obj, n) for n in ('seqid', 'source', 'feature_type', 'score',
                                                       'strand', 'phase')]}
    return model


def _lookup(model, key):
    hit = None
    for name in sorted(model['tables']):
        if key in model['tables'][name]:
            hit = model['tables'][name][key]
    if hit is None:
        raise KeyError(key)
    return hit


def _coords(model, f):
    if f['base']:
        return f['coords']
    if not f['children']:
        return None
    pts = []
    for c in f['children']:
        pts += list(_coords(model, _lookup(model, c)))
    return (min(pts), max(pts))


def _lines(model, f, fmt):
    span = _coords(model, f)
    c = f['cols']
    cols = [c[0], c[1], c[2], str(span[0]), str(span[1]), c[3], c[4], c[5]]  # None: TypeError
    if fmt == 'gtf':
        if not f['base']:
            own = []
        else:
            own = ['\t'.join(cols + ['transcript_id ' + f['parent'] + ';gene_id '
                                     + _lookup(model, f['parent'])['parent']])]
    else:
        tag = 'ID=' + f['ID'] + (';Parent=' + f['parent'] if f['parent'] is not None else '')
        own = ['\t'.join(cols + [tag])]
        if fmt == 'exon added gff3' and f['base'] and c[2] == 'CDS':
            own = [own[0].replace('\tCDS\t', '\texon\t').replace('ID=', 'ID=ExonOf')] + own
    if f['base']:
        return own
    kids = {}
    for cid in f['children']:
        child = _lookup(model, cid)
        key = _coords(model, child)
        if key in kids:
            key = (key[0], key[1] + len(kids))
        kids[key] = _lines(model, child, fmt)
    for key in sorted(kids):
        own += kids[key]
    if fmt == 'exon added gff3':
        for line in own[:]:
            if line.split('\t')[2] == 'CDS':
                own.remove(line)
                own.append(line)
    return own


def write_model(model, fmt, order):
    """write_gff over the field model; raises what the reference raises."""
    names = list(model['names'])
    if order == 'py2':
        names = py2_names(names, model['copies'])
    out = []
    for name in names:
        table = model['tables'].get(name)
        if not table:
            continue
        keys = list(table)
        if order == 'py2':
            keys = py2_keys(keys, model['copies'])
        if table[keys[0]]['parent'] is None:
            for k in keys:
                out.append('\n'.join(_lines(model, table[k], fmt)))
    return '\n'.join(out)


# ---------------------------------------------------------------------------
# Cases and recorded reference runs
# ---------------------------------------------------------------------------

def _g3(seqid, source, ftype, lo, hi, score, strand, phase, tags):
    return '\t'.join([seqid, source, ftype, str(lo), str(hi), score, strand, phase, tags]) + '\n'


def _gene(n, seqid='c1', cds=((10, 50), (80, 120)), score='.', strand='+', source='src'):
    g, t = 'g%d' % n, 't%d' % n
    out = _g3(seqid, source, 'gene', 1, 500, '.', strand, '.', 'ID=' + g)
    out += _g3(seqid, source, 'mRNA', 1, 500, score, strand, '.', 'ID=%s;Parent=%s' % (t, g))
    for k, (lo, hi) in enumerate(cds):
        out += _g3(seqid, source, 'CDS', lo, hi, score, strand, str(k % 3),
                   'ID=%s.c%d;Parent=%s' % (t, k, t))
    return out


def _gtf(seqid, ftype, lo, hi, score, strand, phase, gene, tx=None, source='src'):
    tags = 'gene_id "%s";' % gene + (' transcript_id "%s";' % tx if tx else '')
    return '\t'.join([seqid, source, ftype, str(lo), str(hi), score, strand, phase, tags]) + '\n'


def cases():
    """name -> {'gff': text, 'path': the path every output format takes on a
    machine with a device: 'native', or why the object path runs}.  A dict under
    'path' gives one note per output format."""
    c = {}
    c['gff3_two_genes'] = {'gff': _gene(1) + _gene(2, 'c2', ((300, 400), (5, 9), (100, 200)),
                                                   '0.50', '-'), 'path': 'native'}
    c['gff3_scores'] = {'gff': ''.join(
        _g3('c1', 's', 'gene', 1, 9, '.', '+', '.', 'ID=G%d' % k)
        + _g3('c1', 's', 'mRNA', 1, 9, sc, '+', ph, 'ID=T%d;Parent=G%d' % (k, k))
        + _g3('c1', 's', 'CDS', k + 1, k + 5, sc, '+', ph, 'ID=C%d;Parent=T%d' % (k, k))
        for k, (sc, ph) in enumerate([('1', '0'), ('0.50', '1'), ('-0', '2'), ('.', '.'),
                                      ('', '3'), ('-', ''), ('007', '0'), ('.5', '1'),
                                      ('123456789012', '2'), ('-12.3400', '.'),
                                      ('0.0001', '0'), ('1.', '00')])), 'path': 'native'}
    c['gtf_two_transcripts'] = {'gff': (
        _gtf('c1', 'CDS', 10, 50, '.', '+', '0', 'gA', 'tA1') +
        _gtf('c1', 'exon', 10, 50, '.', '+', '.', 'gA', 'tA1') +
        _gtf('c1', 'CDS', 80, 120, '3.5', '+', '1', 'gA', 'tA1') +
        _gtf('c1', 'CDS', 10, 50, '.', '+', '0', 'gA', 'tA2') +
        _gtf('c1', 'CDS', 200, 250, '.', '+', '2', 'gA', 'tA2') +
        _gtf('c2', 'CDS', 7, 9, '.', '-', '0', 'gB', 'tB1')), 'path': 'native'}
    # three children of equal coords: the third's clash key (10, 52) is free; then a child at
    # (10, 51): the second one's clash key (10, 50 + 1) is taken by it later, and a fourth equal
    # child lands on (10, 50 + 3) = (10, 53)
    c['sibling_clash'] = {'gff': (
        _g3('c1', 's', 'gene', 1, 99, '.', '+', '.', 'ID=g') +
        _g3('c1', 's', 'mRNA', 1, 99, '.', '+', '.', 'ID=t;Parent=g') +
        _g3('c1', 's', 'CDS', 10, 50, '1', '+', '0', 'ID=a;Parent=t') +
        _g3('c1', 's', 'CDS', 10, 51, '2', '+', '0', 'ID=b;Parent=t') +
        _g3('c1', 's', 'CDS', 10, 50, '3', '+', '0', 'ID=c;Parent=t') +
        _g3('c1', 's', 'CDS', 10, 52, '4', '+', '0', 'ID=d;Parent=t') +
        _g3('c1', 's', 'CDS', 10, 50, '5', '+', '0', 'ID=e;Parent=t') +
        _g3('c1', 's', 'CDS', 10, 50, '6', '+', '0', 'ID=f;Parent=t')), 'path': 'native'}
    c['clash_overwrites'] = {'gff': (
        _g3('c1', 's', 'gene', 1, 99, '.', '+', '.', 'ID=g') +
        _g3('c1', 's', 'mRNA', 1, 99, '.', '+', '.', 'ID=t;Parent=g') +
        _g3('c1', 's', 'CDS', 10, 50, '1', '+', '0', 'ID=a;Parent=t') +
        _g3('c1', 's', 'CDS', 10, 52, '2', '+', '0', 'ID=b;Parent=t') +
        _g3('c1', 's', 'CDS', 10, 50, '3', '+', '0', 'ID=c;Parent=t')), 'path': 'native'}
    c['identical_cds_lines'] = {'gff': (
        _g3('c1', 's', 'gene', 1, 99, '.', '+', '.', 'ID=g') +
        _g3('c1', 's', 'mRNA', 1, 99, '.', '+', '.', 'ID=t;Parent=g') +
        _g3('c1', 's', 'CDS', 10, 50, '.', '+', '0', 'ID=x;Parent=t') * 4 +
        _g3('c1', 's', 'mRNA', 1, 99, '.', '+', '.', 'ID=u;Parent=g') +
        _g3('c1', 's', 'CDS', 60, 70, '.', '+', '0', 'ID=y;Parent=u')), 'path': 'native'}
    c['shadowing_attribute'] = {'gff': _gene(1) + _g3('c1', 's', 'CDS', 130, 140, '.', '+', '0',
                                                      'ID=z;Parent=t1;score=9'),
                                'path': 'write_gff takes a diagnostic path'}
    c['crlf_line_ends'] = {'gff': _gene(1).replace('\n', '\r\n'), 'path': 'native'}
    c['cr_in_a_column'] = {'gff': _gene(1).replace('\tsrc\t', '\tsr\rc\t'),
                           'path': 'write_gff takes a diagnostic path'}
    c['source_named_cds'] = {'gff': _gene(1, source='CDS'),
                             'path': {'gff3': 'native', 'gtf': 'native',
                                      'exon_added_gff3': 'write_gff takes a diagnostic path'}}
    # version 2 is fixed by the first line; a later quoted value may hold '='
    c['parent_holds_id_equals'] = {'gff': (
        _gtf('c1', 'CDS', 10, 50, '.', '+', '0', 'gA', 'tA1') +
        _gtf('c1', 'CDS', 80, 120, '.', '+', '1', 'gA', 'tID=2')),
        'path': {'gff3': 'native', 'gtf': 'native',
                 'exon_added_gff3': 'write_gff takes a diagnostic path'}}
    c['regions_beside_genes'] = {'gff': (
        _g3('c1', 's', 'region', 1, 1000, '.', '+', '.', 'ID=r1') + _gene(1) +
        _g3('c2', 's', 'region', 1, 2000, '.', '+', '.', 'ID=r2') + _gene(2, 'c2') +
        _g3('c3', 's', 'chromosome', 1, 9, '.', '.', '.', 'ID=lonely')),
        'path': {'gff3': 'write_gff takes a diagnostic path',
                 'gtf': 'write_gff takes a diagnostic path',
                 'exon_added_gff3': 'write_gff takes a diagnostic path'}}
    c['regions_and_genes_whole'] = {'gff': (
        _g3('c1', 's', 'region', 1, 1000, '.', '+', '.', 'ID=r1') + _gene(1) +
        _g3('c2', 's', 'region', 1, 2000, '7', '-', '1', 'ID=r2') + _gene(2, 'c2')),
        'path': {'gff3': 'native', 'gtf': 'write_gff takes a diagnostic path',
                 'exon_added_gff3': 'native'}}
    c['gene_id_only_gtf'] = {'gff': (_gtf('c1', 'CDS', 10, 50, '.', '+', '0', 'gA') +
                                      _gtf('c1', 'CDS', 80, 90, '.', '+', '0', 'gA')),
                             'path': {'gff3': 'native',
                                      'gtf': 'write_gff takes a diagnostic path',
                                      'exon_added_gff3': 'native'}}
    c['exponent_score'] = {'gff': _gene(1, score='1e-3'), 'path': 'score'}
    c['no_accepted_line'] = {'gff': '# nothing\nshort\tline\n', 'path': 'native'}
    return c


def path_note(case, output_format):
    note = case['path']
    return note[output_format] if isinstance(note, dict) else note


def load():
    with open(GOLDEN) as fh:
        return json.load(fh)
