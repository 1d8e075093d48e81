"""What heterozygosity_from_vcf must give (magot_variants.py:16-139), restated
without magot_amd.magot_variants: ``expected`` (the three prints, the returned
string, the exception name), ``table`` (the device tables: per data line POS,
key hash, het bits, kept and first flags, and the counts per locus),
``native_note`` (which path answers, from the native grammar as the issue
states it), the recorded cases and the seeded worlds of the device tests.

Text is latin-1 str here; files are its bytes."""

import json
import os
import random

from magot_amd import py2order

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, 'golden')
ORDERS = ('py2', 'insertion')
TEXT_BLOCK = 4096  # bytes per workgroup of the line index
INT_MAX = (1 << 31) - 1
PY_SPACE = ' \t\n\r\x0b\x0c'
NO_GT = object()


def load():
    with open(os.path.join(GOLDEN, 'vcf.json')) as fh:
        return json.load(fh)


def py2_int(text):
    s = text.strip(PY_SPACE)
    digits = s[1:] if s[:1] in ('+', '-') else s
    if not digits or not all(c in '0123456789' for c in digits):
        raise ValueError(text)
    return int(s)


def py2_float_str(value):
    text = '%.12g' % value
    return text if ('.' in text or 'e' in text) else text + '.0'


def py2_repr(s):
    quote = '"' if ("'" in s and '"' not in s) else "'"
    esc = {'\\': '\\\\', '\t': '\\t', '\n': '\\n', '\r': '\\r', quote: '\\' + quote}
    return quote + ''.join(esc.get(c, c if 0x20 <= ord(c) < 0x7f else '\\x%02x' % ord(c))
                           for c in s) + quote


def keys_in_order(keys, order, copies=0):
    """distinct keys as a Python 2 dict (or set) built from them iterates after
    ``copies`` rebuilds, or as first seen"""
    if order == 'py2':
        return py2order.order_after_copies(list(keys), copies)
    return list(dict.fromkeys(keys))


# ---------------------------------------------------------------------------
# the model
# ---------------------------------------------------------------------------

def read(text):
    """(the '##' lines, key -> names in insertion order with each one's GT, or
    None for a line without sample fields); raises what read_vcf raises."""
    headers, variants = [], {}
    names = None
    for line in text.replace('\r', '').split('\n'):
        if line == '':
            continue
        if line.startswith('##'):
            headers.append(line)
            continue
        if line.startswith('#'):
            f = line[1:].split('\t')
            if len(f) > 8:
                names = f[9:]
            continue
        f = line.split('\t')
        if len(f) < 8:
            raise IndexError('a data line with fewer than 8 fields')
        key = f[0] + '<:>' + f[1]
        if key not in variants:
            variants[key] = None  # keeps its first place
        variants[key] = None
        if len(f) > 8:
            fmt = f[8].split(':')
            calls = {}
            for column in f[9:]:
                if names is None:
                    raise UnboundLocalError('sample_names')
                who = names[f.index(column) - 9]  # IndexError
                sub = column.split(':')
                gt = NO_GT
                if 'GT' in fmt and fmt.index('GT') < len(sub):
                    gt = sub[fmt.index('GT')]
                calls[who] = gt
            variants[key] = calls
    return headers, variants


def header_loci(headers, window):
    loci = []
    for line in headers:
        if '##contig=<ID=' not in line:
            continue
        parts = line.split(',')
        seqid, seqlen = parts[0][13:], py2_int(parts[1][7:-1])
        full = seqlen // window
        loci += ['%s,%d,%d' % (seqid, 1 + window * k, window * (k + 1)) for k in range(full)]
        loci.append('%s,%d,%d' % (seqid, 1 + window * full, seqlen))
    return loci


def expected(text, loci=None, window=10000, order='py2'):
    """(stdout, returned string or None, exception name or None)"""
    out = []
    try:
        ret = _expected(text, loci, window, order, out)
        return ''.join(s + '\n' for s in out), ret, None
    except Exception as e:  # noqa: BLE001
        return ''.join(s + '\n' for s in out), None, type(e).__name__


def _expected(text, loci, window, order, out):
    headers, variants = read(text)
    if loci is None:
        loci = header_loci(headers, window)
    loci = keys_in_order(loci, order)
    out += ['built locus list', str(len(loci))]
    codes = keys_in_order(variants, order)
    counts, by_seqid = {}, {}
    for locus in loci:
        counts[locus] = dict.fromkeys(variants[codes[0]], 0)
        by_seqid.setdefault(locus.split(',')[0], []).append(locus)
    for code in codes:
        seqid, position = code.split('<:>')[0], py2_int(code.split('<:>')[1])
        for locus in by_seqid[seqid]:
            f = locus.split(',')
            if len(f) > 2 and not py2_int(f[1]) <= position <= py2_int(f[2]):
                continue
            for who in variants[code]:  # a line without sample fields: TypeError
                gt = variants[code][who]
                if gt is NO_GT:
                    raise AttributeError('GT')
                if gt[0] != gt[-1]:
                    counts[locus][who] += 1
    rows, std = [], None
    for locus in loci:
        if std is None:
            std = keys_in_order(counts[locus], order, copies=2)
            out.append('[' + ', '.join(py2_repr(n) for n in std) + ']')
        f = locus.split(',')
        seqlen = py2_int(f[2]) - py2_int(f[1]) + 1 if len(f) > 2 else py2_int(f[1])
        if seqlen >= 1:
            rows.append(','.join([locus] + [py2_float_str(100.0 * counts[locus][n] / seqlen)
                                            for n in std]))
    return '\n'.join(rows)


# ---------------------------------------------------------------------------
# the native grammar and the device tables
# ---------------------------------------------------------------------------

def split_lines(text):
    """[(0-based line, its text without LF)]: a text that ends in LF has no
    empty last line"""
    lines = text.split('\n')
    if lines and lines[-1] == '':
        lines.pop()
    return list(enumerate(lines))


def _line_reason(f, n_samples):
    if len(f) != 9 + n_samples:
        return 'field_count'
    if '<:>' in f[0]:
        return 'chrom_form'
    pos = f[1]
    if not pos or not all(c in '0123456789' for c in pos) or (len(pos) > 1 and pos[0] == '0'):
        return 'pos_form'
    if len(pos) > 10 or int(pos) > INT_MAX:
        return 'pos_range'
    fmt = f[8].split(':')
    if 'GT' not in fmt:
        return 'no_gt'
    gi = fmt.index('GT')
    if any(len(c.split(':')) <= gi or c.split(':')[gi] == '' for c in f[9:]):
        return 'empty_gt'
    if any(f.index(c) < 9 for c in f[9:]):
        return 'equals_fixed'
    return None


def loci_ok(loci):
    for locus in loci:
        f = locus.split(',')
        nums = f[1:3]
        if len(f) < 2:
            return False
        for x in nums:
            digits = x[1:] if x[:1] == '-' else x
            if not digits or len(digits) > 18 or not all(c in '0123456789' for c in digits):
                return False
    return True


def native_note(text, loci=None, window=10000, order='py2'):
    """'native', 'raise' (the device path raises the KeyError of a CHROM without
    a locus itself) or the reason the device path declines for"""
    if '\r' in text:
        return 'carriage_return'
    lines = split_lines(text)
    head = [k for k, ln in lines if ln[:1] == '#' and ln[:2] != '##']
    data = [(k, ln.split('\t')) for k, ln in lines if ln and ln[0] != '#']
    if not head:
        return 'no_header'
    if len(head) > 1:
        return 'many_headers'
    if not data:
        return 'no_data'
    if data[0][0] < head[0]:
        return 'header_after_data'
    names = lines[head[0]][1][1:].split('\t')[9:]
    if not names:
        return 'no_samples'
    for _, f in data:
        why = _line_reason(f, len(names))
        if why:
            return why
    if len(set(names)) != len(names):
        return 'duplicate_names'
    if loci is None:
        try:
            loci = header_loci([ln for _, ln in lines if ln[:2] == '##'], window)
        except (ValueError, IndexError, ZeroDivisionError):
            return 'header_form'
    if not all(isinstance(x, str) for x in loci) or not loci_ok(loci):
        return 'locus_form'
    seqids = {locus.split(',')[0] for locus in loci}
    if any(f[0] not in seqids for _, f in data):
        return 'raise'
    t = table(text, keys_in_order(loci, order), order)
    return 'foreign_name' if t['foreign'] else 'native'


def table(text, loci, order):
    """For a text inside the native grammar and loci of plain numbers: per data
    line 'line', 'pos', 'hash', 'bits' (a Python int, bit s for sample column s),
    'kept', 'first'; 'contig_of_run'; 'first_line' (the line of
    list(variant_set)[0]); 'allowed' (an int); 'counts' (per locus a list per
    sample column) and 'foreign'."""
    lines = split_lines(text)
    data = [(k, ln.split('\t')) for k, ln in lines if ln and ln[0] != '#']
    n_samples = len(data[0][1]) - 9
    seq_ids = {}
    for locus in loci:
        seq_ids.setdefault(locus.split(',')[0], len(seq_ids))
    t = {'line': [], 'pos': [], 'hash': [], 'bits': [], 'key': [], 'runs': []}
    for k, f in data:
        gi = f[8].split(':').index('GT')
        bits = 0
        for s, column in enumerate(f[9:]):
            gt = column.split(':')[gi]
            if f.index(column) == 9 + s and gt[0] != gt[-1]:
                bits |= 1 << s
        t['line'].append(k)
        t['pos'].append(int(f[1]))
        t['hash'].append(py2order.str_hash(f[0] + '<:>' + f[1]))
        t['bits'].append(bits)
        t['key'].append((f[0], int(f[1])))
        if not t['runs'] or t['runs'][-1] != f[0]:
            t['runs'].append(f[0])
    t['contig_of_run'] = [seq_ids.get(name) for name in t['runs']]
    last_of, first_of = {}, {}
    for d, key in enumerate(t['key']):
        last_of[key] = d
        first_of.setdefault(key, d)
    t['kept'] = [int(last_of[key] == d) for d, key in enumerate(t['key'])]
    t['first'] = [int(first_of[key] == d) for d, key in enumerate(t['key'])]
    codes = keys_in_order(['%s<:>%d' % key for key in first_of], order)
    chrom, _, pos = codes[0].rpartition('<:>')
    d0 = last_of[(chrom, int(pos))]
    t['first_line'] = t['line'][d0]
    f0 = data[d0][1]
    t['allowed'] = 0
    for column in f0[9:]:
        t['allowed'] |= 1 << (f0.index(column) - 9)
    t['counts'], t['foreign'] = [], False
    for locus in loci:
        f = locus.split(',')
        row = [0] * n_samples
        for d, (chrom, pos) in enumerate(t['key']):
            if not t['kept'][d] or chrom != f[0]:
                continue
            if len(f) > 2 and not int(f[1]) <= pos <= int(f[2]):
                continue
            if t['bits'][d] & ~t['allowed']:
                t['foreign'] = True
            for s in range(n_samples):
                row[s] += t['bits'][d] >> s & 1
        t['counts'].append(row)
    return t


# ---------------------------------------------------------------------------
# the recorded cases
# ---------------------------------------------------------------------------

def vcf(lines, names=('s1', 's2', 's3'), contigs=(('c1', 25000),), end='\n', final=True):
    """a VCF text: ##fileformat, a ##contig line per contig, the '#' line for
    ``names``, then ``lines`` (each a list of fields or a str)"""
    head = ['##fileformat=VCFv4.2']
    head += ['##contig=<ID=%s,length=%d>' % c for c in contigs]
    head.append('\t'.join(['#CHROM', 'POS', 'ID', 'REF', 'ALT', 'QUAL', 'FILTER', 'INFO', 'FORMAT']
                          + list(names)))
    body = [ln if isinstance(ln, str) else '\t'.join(ln) for ln in lines]
    text = end.join(head + body)
    return text + end if final else text


def row(chrom, pos, *calls, **kw):
    return [chrom, str(pos), kw.get('id', 'rs%s' % pos), 'A', 'C', '50', 'PASS',
            kw.get('info', 'DP=9'), kw.get('fmt', 'GT:DP')] + list(calls)


def cases():
    """name -> (text, loci or None, window)"""
    c = {}
    c['plain'] = (vcf([row('c1', 5, '0/1:5', '0/0:6', '1/1:7'),
                       row('c1', 10001, '0/0:5', '0/1:6', '1/2:7'),
                       row('c1', 10002, '0|1:5', '1|0:6', '1|1:7'),
                       row('c1', 24999, '0/1:3', '0/1:4', '0/1:8')]), None, 10000)
    c['het_quirks'] = (vcf([row('c1', 7, '1:5', './.:6', '10/1:7'),
                            row('c1', 8, '1/2:5', '0/1:6', '.:7'),
                            row('c1', 9, '2/1/2:5', '01:6', '0/10:7')]), None, 10000)
    # two equal columns on a later line: the later sample is absent there
    c['dup_columns_later'] = (vcf([row('c1', 5, '0/1:5', '0/0:6', '1/1:7'),
                                   row('c1', 6, '0/1:5', '0/1:6', '0/1:5')]), ['c1,1,100'], 10000)
    # ... on the line of the first variant: a het of 's2' elsewhere is a KeyError
    c['dup_columns_first'] = (vcf([row('c1', 5, '0/1:5', '0/1:5', '1/1:7'),
                                   row('c1', 6, '0/1:5', '0/1:6', '0/1:7')]), ['c1,1,100'], 10000)
    c['dup_columns_first_no_het'] = (vcf([row('c1', 5, '0/1:5', '0/1:5', '1/1:7')]),
                                     ['c1,1,100'], 10000)
    c['column_equals_id'] = (vcf([row('c1', 5, '.', '0/1', '1/1', id='.', fmt='GT')]),
                             ['c1,1,100'], 10000)
    c['same_key_adjacent'] = (vcf([row('c1', 5, '0/1:5', '0/0:6', '1/1:7'),
                                   row('c1', 5, '0/0:5', '0/1:6', '1/1:7'),
                                   row('c1', 6, '0/1:5', '0/0:6', '0/1:7')]), None, 10000)
    c['same_key_far'] = (vcf([row('c1', 5, '0/1:5', '0/0:6', '1/1:7'),
                              row('c2', 5, '0/1:5', '0/1:6', '0/1:7'),
                              row('c1', 9, '0/0:5', '0/0:6', '0/1:7'),
                              row('c1', 5, '1/1:5', '0/1:6', '0/1:7')],
                             contigs=(('c1', 25000), ('c2', 9000))), None, 10000)
    c['interleaved_contigs'] = (vcf([row('c1', 5, '0/1:5', '0/0:6', '1/1:7'),
                                     row('c2', 7, '0/1:5', '0/1:6', '0/1:7'),
                                     row('c1', 12000, '0/1:5', '0/1:6', '0/1:7'),
                                     row('c2', 8, '0/0:5', '0/1:6', '0/1:7'),
                                     row('c1', 6, '0/1:5', '0/0:6', '0/1:7')],
                                    contigs=(('c1', 25000), ('c2', 9000))), None, 10000)
    c['gt_second'] = (vcf([row('c1', 5, '5:0/1', '6:0/0', '7:1/2', fmt='DP:GT'),
                           row('c1', 6, '5:0/0', '6:0/1', '7:1/1', fmt='DP:GT')]), None, 10000)
    c['format_changes'] = (vcf([row('c1', 5, '5:0/1', '6:0/0', '7:1/2', fmt='DP:GT'),
                                row('c1', 6, '0/1', '0/1', '1/1', fmt='GT'),
                                row('c1', 7, '0/1:5:9', '0/0:6:9', '1/0:7:9', fmt='GT:DP:GQ')]),
                           None, 10000)
    c['gt_twice_in_format'] = (vcf([row('c1', 5, '0/1:1/1', '0/0:0/1', '1/1:0/1', fmt='GT:GT')]),
                               None, 10000)
    c['crlf'] = (vcf([row('c1', 5, '0/1', '0/0', '0/1', fmt='GT'),
                      row('c1', 6, '0/1', '0/1', '1/1', fmt='GT')], end='\r\n'), None, 10000)
    c['lone_cr'] = (vcf([row('c1', 5, '0/1:5', '0/0:6', '0/\r1:7')]), None, 10000)
    c['no_final_lf'] = (vcf([row('c1', 5, '0/1:5', '0/0:6', '1/1:7'),
                             row('c1', 6, '0/1:5', '0/1:6', '1/0:7')], final=False), None, 10000)
    text = vcf([row('c1', 5, '0/1:5', '0/0:6', '1/1:7'), '', '##note=in the middle',
                row('c1', 6, '0/1:5', '0/1:6', '1/0:7'), '',
                '##contig=<ID=c9,length=12>', ''])
    c['blank_and_header_lines_inside'] = (text + '\n', None, 10000)
    w = 100
    c['window_edges'] = (vcf([row('c1', p, '0/1:5', '0/0:6', '1/0:7')
                              for p in (0, 1, w, w + 1, 2 * w, 2 * w + 1, 250, 251, 252)],
                             contigs=(('c1', 251),)), None, w)
    c['seqlen_multiple_of_window'] = (vcf([row('c1', p, '0/1:5', '0/0:6', '1/0:7')
                                           for p in (1, 100, 101, 200, 201)],
                                          contigs=(('c1', 200),)), None, 100)
    c['seqlen_below_window'] = (vcf([row('c1', p, '0/1:5', '0/0:6', '1/0:7') for p in (1, 30, 31)],
                                    contigs=(('c1', 30),)), None, 100)
    c['contig_header_twice'] = (vcf([row('c1', 5, '0/1:5', '0/0:6', '1/1:7')],
                                    contigs=(('c1', 250), ('c1', 250), ('c2', 90))), None, 100)
    text = vcf([row('c1', 5, '0/1:5', '0/0:6', '1/1:7'), row('c1', 2000, '0/1:5', '0/1:6', '1/1:7')])
    c['contig_header_third_attribute'] = (
        text.replace('length=25000>', 'length=2500,assembly=b37>'), None, 1000)
    c['contig_header_no_length'] = (text.replace(',length=25000>', '>'), None, 1000)
    many = [row('c1', p, '0/1:5', '0/0:6', '1/0:7') for p in (1, 5, 10, 11, 50, 99, 100)]
    c['loci_overlap'] = (vcf(many), ['c1,1,10', 'c1,5,50', 'c1,10,10', 'c1,1,100', 'c1,5,50'], 10000)
    c['loci_two_fields'] = (vcf(many + [row('c2', 3, '0/1:5', '0/1:6', '1/1:7')]),
                            ['c1,250', 'c2,7', 'c1,1,10'], 10000)
    c['loci_start_after_stop'] = (vcf(many), ['c1,50,10', 'c1,11,10', 'c1,1,10', 'c1,0', 'c1,-5'],
                                  10000)
    c['loci_negative_and_huge'] = (vcf(many), ['c1,-5,5', 'c1,99,5000000000', 'c1,3000000000,3000000001'],
                                   10000)
    c['loci_lack_a_seqid'] = (vcf(many + [row('c2', 3, '0/1:5', '0/1:6', '1/1:7')]), ['c1,1,10'],
                              10000)
    c['loci_empty'] = (vcf(many), [], 10000)
    c['loci_malformed'] = (vcf(many), ['c1,1,x'], 10000)
    c['loci_one_field'] = (vcf(many), ['c1'], 10000)
    c['no_variants'] = (vcf([]), None, 10000)
    c['no_variants_no_loci'] = (vcf([], contigs=()), None, 10000)
    c['no_header_line'] = ('##fileformat=VCFv4.2\n##contig=<ID=c1,length=100>\n' +
                           '\t'.join(row('c1', 5, '0/1:5')) + '\n', None, 10000)
    c['eight_fields'] = (vcf([row('c1', 5)[:8]]), None, 10000)
    c['eight_fields_later'] = (vcf([row('c1', 5, '0/1:5', '0/0:6', '1/1:7'), row('c1', 6)[:8]]),
                               None, 10000)
    c['seven_fields'] = (vcf([row('c1', 5)[:7]]), None, 10000)
    c['short_line'] = (vcf([row('c1', 5, '0/1:5', '0/0:6')]), None, 10000)
    c['long_line'] = (vcf([row('c1', 5, '0/1:5', '0/0:6', '1/1:7', '0/1:8')]), None, 10000)
    c['sample_without_gt'] = (vcf([row('c1', 5, '5:0/1', '6', '7:1/1', fmt='DP:GT')]), None, 10000)
    c['empty_gt'] = (vcf([row('c1', 5, '0/1:5', ':6', '1/1:7')]), None, 10000)
    c['format_without_gt'] = (vcf([row('c1', 5, '5', '6', '7', fmt='DP')]), None, 10000)
    c['pos_leading_zero'] = (vcf([row('c1', '05', '0/1:5', '0/0:6', '1/1:7')]), None, 10000)
    c['pos_not_a_number'] = (vcf([row('c1', 'x5', '0/1:5', '0/0:6', '1/1:7')]), None, 10000)
    c['pos_beyond_int32'] = (vcf([row('c1', 1 << 31, '0/1:5', '0/0:6', '1/1:7')]),
                             ['c1,1,3000000000'], 10000)
    c['pos_at_int32'] = (vcf([row('c1', INT_MAX, '0/1:5', '0/0:6', '1/1:7')]),
                         ['c1,1,3000000000', 'c1,2147483647,2147483647', 'c1,2147483648,2147483649'],
                         10000)
    c['chrom_holds_the_separator'] = (vcf([row('c<:>1', 5, '0/1:5', '0/0:6', '1/1:7')]),
                                      ['c,1,10'], 10000)
    c['names_repeat'] = (vcf([row('c1', 5, '0/1:5', '0/0:6', '1/0:7')], names=('s1', 's2', 's1')),
                         None, 10000)
    c['header_line_twice'] = (vcf(['#CHROM\tPOS', row('c1', 5, '0/1:5', '0/0:6', '1/0:7')]),
                              None, 10000)
    c['header_after_data'] = ('##contig=<ID=c1,length=100>\n' + '\t'.join(row('c1', 5, '0/1:5'))
                              + '\n' + vcf([row('c1', 6, '0/1:5', '0/0:6', '1/0:7')]), None, 10000)
    c['one_sample'] = (vcf([row('c1', 5, '0/1:5'), row('c1', 6, '0/0:5'), row('c1', 7, '1/0:5')],
                           names=('only',)), None, 10000)
    c['names_to_escape'] = (vcf([row('c1', 5, '0/1:5', '0/0:6', '1/0:7')],
                                names=("it's", 'a"b\'c', 'caf\xe9\\')), None, 10000)
    rnd = random.Random(20261020)
    for k in range(6):
        c['random_%d' % k] = (random_text(rnd), None, rnd.choice([50, 100, 1000]))
    return c


def random_text(rnd, n_samples=None, n_lines=None):
    """a small text inside the native grammar: three contigs, repeated keys,
    repeated columns, every sample named by every first variant"""
    n_samples = n_samples or rnd.randint(1, 40)
    n_lines = n_lines or rnd.randint(1, 60)
    contigs = (('chrA', rnd.randint(1, 999)), ('chrB', rnd.randint(1, 999)), ('c', 100))
    gts = ['0/0', '0/1', '1/1', '1/2', './.', '1', '10/1', '0|1', '1|0']
    lines = []
    for _ in range(n_lines):
        chrom, length = rnd.choice(contigs)
        pos = rnd.choice([0, 1, length, length + 1, rnd.randint(1, length)])
        # distinct columns: the depth is the sample's own number
        lines.append(row(chrom, pos, *['%s:%d' % (rnd.choice(gts), s) for s in range(n_samples)]))
    return vcf(lines, names=['n%d' % s for s in range(n_samples)], contigs=contigs)


# ---------------------------------------------------------------------------
# the seeded worlds of the device tests
# ---------------------------------------------------------------------------

LINE_COUNTS = (1, 63, 64, 65, 255, 256, 257, 4099)
SAMPLE_COUNTS = (1, 2, 31, 32, 33, 64, 65, 130)
WORLDS = ([(n, 3) for n in LINE_COUNTS] + [(257, s) for s in SAMPLE_COUNTS] + [(4099, 65)])
_GTS = ('0/0', '0/1', '1/1', '1/2', './.', '1', '10/1', '0|1', '1|0', '2/1/2')
_worlds = {}


def world(n_data, n_samples, seed=20261020):
    """(text, loci): n_data data lines of n_samples columns.  Runs of CHROM:
    one line of A, one of B, A again for all lines but the last, which is C's
    (with 4 lines and more); one INFO above 8192 bytes; keys repeat;
    columns repeat within a line; a '##' line is cut so that a line starts at a
    multiple of TEXT_BLOCK.  The loci: windows and overlaps on A, the whole of
    A, of B and of C, and one locus that holds nothing."""
    if (n_data, n_samples, seed) in _worlds:
        return _worlds[(n_data, n_samples, seed)]
    rnd = random.Random(seed * 1000003 + n_data * 131 + n_samples)
    if n_data < 4:
        chroms = ['ctgA', 'ctgB', 'ctgC'][:n_data]
    else:
        chroms = ['ctgA', 'ctgB'] + ['ctgA'] * (n_data - 3) + ['ctgC']
    top = max(3 * n_data, 10)
    lines, used = [], []
    for d, chrom in enumerate(chroms):
        pos = rnd.randint(0, top)
        if used and rnd.random() < 0.2:
            pos = rnd.choice(used)[1]  # a position again: a key again where the CHROM is the same
        used.append((chrom, pos))
        calls = []
        for s in range(n_samples):
            if calls and rnd.random() < 0.15:
                calls.append(rnd.choice(calls))
            else:
                calls.append('%s:%d' % (rnd.choice(_GTS), rnd.randint(1, 30)))
        fmt = 'GT:DP'
        if rnd.random() < 0.2:
            fmt, calls = 'DP:GT', [':'.join(reversed(c.split(':'))) for c in calls]
        info = 'DP=9'
        if d == n_data // 2:
            info = 'LONG=' + 'x' * 9000
        lines.append(row(chrom, pos, *calls, fmt=fmt, info=info))
    names = ['smp%d' % s for s in range(n_samples)]
    contigs = (('ctgA', top + 1), ('ctgB', 77), ('ctgC', top))
    text = vcf(lines, names=names, contigs=contigs)
    # the first data line starts at a multiple of TEXT_BLOCK, by a '##' line of
    # the right length
    first = text.index('\nctgA\t') + 1
    pad = (-first) % TEXT_BLOCK
    if pad < 7:
        pad += TEXT_BLOCK
    text = '##pad=' + 'p' * (pad - 7) + '\n' + text
    w = max(top // 7, 1)
    loci = ['ctgA,%d,%d' % (1 + w * k, w * (k + 1)) for k in range(8)]
    loci += ['ctgA,%d' % (top + 1), 'ctgB,77', 'ctgC,%d' % top, 'ctgA,0,%d' % top, 'ctgA,5,4',
             'ctgA,%d,%d' % (top + 5, top + 9), 'ctgB,3,%d' % top, 'ctgA,%d,%d' % (w, 3 * w)]
    _worlds[(n_data, n_samples, seed)] = (text, loci)
    return text, loci
