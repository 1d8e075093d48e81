"""What tab2fasta (genome_tools.py:345-346 over magot_smallfuncs.py:12-18) and
repeatmasker2augustushints (genome_tools.py:449-454) print, restated for the
tests: both loops over bytes, the cut program's model of a line (its verdict,
the bytes it prints, its pieces), the case table recorded in
tests/golden/tabcut.json and seeded tables for the device tests.  Nothing here
imports the code under test."""

import itertools
import json
import os
import random

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, 'golden')
ALIGN = os.path.join(GOLDEN, 'Align.pep.tab')
ALIGN_CKSUM = (925279487, 14901)  # test_data/test_suite.py:10

# what the host tests assume where no device is asked (test_gpu_tabcut.py reads
# engine.TabCut.params())
PARAMS = {'piece': 4096, 'text_block': 4096, 'max_items': 8}

# the two programs: TABs a line must have, what a line with fewer does, the CR
# check, the items (bytes: a literal; a pair: the fields a..b)
TAB2FASTA = dict(need=1, short='error', cr_check=True, items=(b'>', (0, 0), b'\n', (1, 1), b'\n'))
HINTS = dict(need=6, short='skip', cr_check=False,
             items=((0, 1), b'\tnonexonpart\t', (3, 5), b'\t.\t.\tpri=2;src=RM\n'))
SKIPPED, KEPT, SHORT = 0, 1, 2


def load():
    with open(os.path.join(GOLDEN, 'tabcut.json')) as fh:
        return json.load(fh)


def lines_of(data):
    """``for line in open(path)`` of Python 2: lines end after LF only"""
    parts = data.split(b'\n')
    last = parts.pop()
    return [p + b'\n' for p in parts] + ([last] if last else [])


def expected_tab2fasta(data):
    """(stdout, exception name) of the reference's tab2fasta"""
    rows = []
    for line in lines_of(data):
        fields = line.replace(b'\n', b'').replace(b'\r', b'').split(b'\t')
        if len(fields) < 2:
            return b'', 'IndexError'
        rows.append(b'>' + fields[0] + b'\n' + fields[1])
    return b'\n'.join(rows) + b'\n', None


def expected_hints(data):
    """(stdout, exception name) of the reference's repeatmasker2augustushints"""
    out = []
    for line in lines_of(data):
        if line.count(b'\t') > 5:
            f = line.split(b'\t')
            out.append(b'\t'.join([f[0], f[1], b'nonexonpart', f[3], f[4], f[5], b'.', b'.',
                                   b'pri=2;src=RM']) + b'\n')
    return b''.join(out), None


def stray_cr(data):
    """a CR that is neither directly before an LF nor the text's last byte"""
    return any(c == 13 and i + 1 < len(data) and data[i + 1] != 10 for i, c in enumerate(data))


def tab2fasta_path(data):
    """'native', or why the device path of tab2fasta is not taken"""
    return 'stray_cr' if stray_cr(data) else 'native'


def line_model(line, need, items):
    """None for a line with fewer than ``need`` TABs, else the byte strings its
    items print: a field ends at one of the first ``need`` TABs, field ``need``
    at the next TAB or at the line's end less the LF and one CR before it."""
    tabs = [i for i, c in enumerate(line) if c == 9]
    if len(tabs) < need:
        return None
    end = len(line)
    if end and line[end - 1] == 10:
        end -= 1
    if end and line[end - 1] == 13:
        end -= 1
    out = []
    for item in items:
        if isinstance(item, bytes):
            out.append(item)
            continue
        a, b = item
        start = tabs[a - 1] + 1 if a else 0
        stop = tabs[b] if b < need or len(tabs) > need else end
        out.append(line[start:stop])
    return out


def rows_model(data, need, short, items, piece=PARAMS['piece'], **_):
    """The device's tables restated: per line the verdict and the output
    offset; the kept lines, the pieces, the output and the lowest short line."""
    verdict, offset, out, pieces, short_line = [], [], [], 0, None
    at = 0
    for k, line in enumerate(lines_of(data)):
        parts = line_model(line, need, items)
        offset.append(at)
        if parts is None:
            verdict.append(SHORT if short == 'error' else SKIPPED)
            if short == 'error' and short_line is None:
                short_line = k
            continue
        verdict.append(KEPT)
        out.extend(parts)
        at += sum(len(p) for p in parts)
        pieces += sum((len(p) + piece - 1) // piece for p in parts)
    return {'verdict': verdict, 'offset': offset, 'out': b''.join(out), 'n_pieces': pieces,
            'n_kept': verdict.count(KEPT), 'short_line': short_line,
            'n_tabs': data.count(b'\t')}


def _seq(n, salt=0):
    """n bytes of residues, none a TAB, LF or CR, varying with their place"""
    alphabet = b'ACDEFGHIKLMNPQRSTVWY-'
    return bytes(alphabet[(i * 7 + i // 21 + salt) % len(alphabet)] for i in range(n))


def table_of_size(n, with_lf=True):
    """a table of exactly n bytes: 'name TAB residues' lines of uneven lengths"""
    rnd = random.Random(n)
    out = bytearray()
    k = 0
    while len(out) < n - 200:
        out += b'r%d\t' % k + _seq(rnd.randrange(0, 90), k) + b'\n'
        k += 1
    return _filled(out, n, with_lf)


def _filled(out, n, with_lf=True):
    """``out`` and one more line whose second field brings the text to n bytes"""
    out = bytes(out) + b'z\t'
    out += _seq(n - len(out) - (1 if with_lf else 0)) + (b'\n' if with_lf else b'')
    assert len(out) == n
    return out


def straddling_table(block=PARAMS['text_block']):
    """two blocks of text; one line starts in the first and has its TABs in the second"""
    out = bytearray()
    k = 0
    while len(out) + 57 <= block - 10:
        out += b'n%d\t' % k + _seq(50, k) + b'\tx\n'
        k += 1
    out += b'L' * 100 + b'\t' + _seq(30) + b'\t\n'  # its name crosses the block edge
    assert out.rfind(b'\n', 0, len(out) - 1) + 1 < block < out.rfind(b'L') + 1
    while len(out) < 2 * block - 200:
        out += b'n%d\t' % k + _seq(50, k) + b'\n'
        k += 1
    return _filled(out, 2 * block)


def lines_table(n, with_lf):
    text = b''.join(b'q%d\t%s\n' % (k, _seq(k % 7, k)) for k in range(n))
    return text if with_lf else text[:-1]


def field_table(sizes):
    """one line per size: a name of 0..17 bytes by its place, the field of that size"""
    return b''.join(b'N' * (k % 18) + b'\t' + _seq(n, k) + b'\n' for k, n in enumerate(sizes))


def hint_line(n_tabs, tag):
    """a line of n_tabs TABs whose fields name the line and their place"""
    return b'\t'.join(b'%s%d' % (tag, f) for f in range(n_tabs + 1)) + b'\n'


def cases():
    """name -> text.  Every row of the issue's two tables of observed runs,
    then the shapes of the device tests that are small enough to record."""
    c = {
        'empty_file': b'',
        'no_lf': b'a\tb',
        'one_line': b'a\tb\n',
        'crlf': b'a\tb\r\n',
        'cr_at_the_end': b'a\tb\r',
        'third_field_empty_crlf': b'a\tb\t\r\n',
        'third_field': b'a\tb\tc\n',
        'cr_in_fields': b'a\rx\ty\rz\n',
        'only_a_tab': b'\t\n',
        'two_lines_no_lf': b'a\tb\nc\td',
        'no_tab': b'a\n',
        'empty_line': b'\n',
        'empty_last_line': b'a\tb\n\n',
        'six_fields': b'1\t2\t3\t4\t5\t6\n',
        'comment_short_and_no_lf': b'#c\t2\t3\t4\t5\t6\t7\t8\t9\r\nshort\n1\t\t\t\t\t\t',
        'cr_in_hint_fields': b'a\r\tb\t\t\t\t\r\t\n',
    }
    for n in (4095, 4096, 4097, 8192):
        c['size_%d' % n] = table_of_size(n)
    c['size_4096_no_lf'] = table_of_size(4096, with_lf=False)
    c['straddle'] = straddling_table()
    for n in (31, 32, 33, 64, 256):
        c['lines_%d' % n] = lines_table(n, True)
        c['lines_%d_no_lf' % n] = lines_table(n, False)
    c['fields'] = field_table([0, 1, 4095, 4096, 4097, 8192, 8193])
    # tab2fasta writes line k's field at its offset + k % 18 + 2: sized so that each field
    # begins one residue mod 16 behind the last, at least two whole chunks long
    c['names_0_to_17'] = field_table([32 + (-2 - (k + 1) % 18) % 16 for k in range(18)])
    # tab2fasta's pieces: '>' and the two LFs, one for a name, one per 4096 bytes of field 1
    c['pieces_15'] = b'a\tb\n' * 3
    c['pieces_16'] = b'a\t\n' * 4
    c['pieces_17'] = b'a\tb\n' + b'a\t\n' * 3
    c['pieces_33'] = b'a\tb\n' * 5 + b'a\t\n' * 2
    for order in itertools.permutations((5, 6, 7)):
        c['tabs_%d%d%d' % order] = b''.join(hint_line(n, b'f%d_' % n) for n in order)
    c['tabs_5000'] = hint_line(5, b'a') + hint_line(5000, b'w') + hint_line(6, b'b')
    c['tab_is_the_last_byte'] = hint_line(6, b'p') + b'q0\tq1\tq2\tq3\tq4\tq5\t'
    c['last_line_without_tab'] = hint_line(7, b'p') + b'no tab here'
    c['comments_only'] = b'# a comment\n##gff-version 3\n#\tone tab\n'
    c['short_first'] = b'none\na\tb\nc\td\n'
    c['short_last'] = b'a\tb\nc\td\nnone'
    c['short_twice'] = b'a\tb\nnone\nc\td\n\ne\tf\n'
    c['stray_cr_mid_line'] = b'a\tb\nc\rc\td\n'
    return c


def random_table(seed=20261021, n_lines=2000):
    """0 to 9 TABs per line, fields of 0 to 40 bytes, no CR; the last line without LF"""
    rnd = random.Random(seed)
    rows = []
    for _ in range(n_lines):
        rows.append(b'\t'.join(_seq(rnd.randrange(0, 41), rnd.randrange(99))
                               for _ in range(rnd.randrange(0, 10) + 1)))
    return b'\n'.join(rows)
