"""What besthits_from_psl must give (genome_tools.py:572-592): the reference's
loop restated (``expected``), the table engine.BestHits must return and the
native grammar's verdict restated line by line (``table``), the inputs of the
recorded cases (``cases``), the seeded worlds the device tests run on, and the
loader of the reference's own output (tests/golden/psl.json, written by
golden/make_golden_psl.py).  Not a test module: test_psl_host.py,
test_gpu_psl.py and the golden generator import it."""

import json
import os
import random

from magot_amd import py2order

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, 'golden')

PASS_BYTES = (b'p', b'\n', b'm', b'-', b'\t', b' ')
PY_SPACE = b' \t\n\r\x0b\x0c'
TEXT_BLOCK = 4096  # bytes per workgroup of the line index
INT_MAX = (1 << 31) - 1

HEADER = (b'psLayout version 3\n'
          b'\n'
          b'match\tmis- \trep. \tN\'s\tQ gap\tQ gap\tT gap\tT gap\tstrand\tQ   \t'
          b'Q   \tQ    \tQ  \tT   \tT   \tT    \tT  \tblock\tblockSizes \tqStarts\t tStarts\n'
          b'     \tmatch\tmatch\t   \tcount\tbases\tcount\tbases\t      \tname\t'
          b'size\tstart\tend\tname\tsize\tstart\tend\tcount\n'
          b'-----------------------------------------------------------------------------------'
          b'----------------------------------------------------------------------------\n')


def load():
    with open(os.path.join(GOLDEN, 'psl.json')) as fh:
        return json.load(fh)


def lines_of(data):
    """``for line in open(path)`` of Python 2: lines end after LF only"""
    parts = bytes(data).split(b'\n')
    return [p + b'\n' for p in parts[:-1]] + ([parts[-1]] if parts[-1] else [])


def py2_int(field):
    """int() as Python 2 reads a byte string; ValueError otherwise"""
    s = field.strip(PY_SPACE)
    digits = s[1:] if s[:1] in (b'+', b'-') else s
    if not digits or not digits.isdigit():
        raise ValueError(field)
    return int(s)


def expected(data, order):
    """The bytes the reference prints for the PSL text ``data``: the loop of
    genome_tools.py:572-592 restated.  ``order``: 'py2' (the winners in the
    order a Python 2 dict of the first-seen keys iterates) or 'insertion'."""
    out = []
    best = {}
    for line in lines_of(data):
        if line[:1] in PASS_BYTES:
            out.append(line[:-1] + b'\n')
            continue
        fields = line.split(b'\t')
        try:
            key = fields[9]
            score = py2_int(fields[0]) - py2_int(fields[1])
        except (IndexError, ValueError):
            out.append(line + b'\n')
            return b''.join(out)
        if key not in best or score > best[key][0]:
            best[key] = (score, line[:-1])
    keys = list(best)
    if order == 'py2':
        keys = [k.encode('latin-1')
                for k in py2order.dict_order([k.decode('latin-1') for k in keys])]
    else:
        assert order == 'insertion'
    return b''.join(out + [best[k][1] + b'\n' for k in keys])


class Decline(Exception):
    pass


def _native_field(field):
    """The native grammar of field 0 and field 1: 1 to 10 digits alone, at
    most 2^31 - 1.  Form is judged before range."""
    if not field or not all(48 <= c <= 57 for c in field):
        raise Decline('integer_form')
    if len(field) > 10 or int(field) > INT_MAX:
        raise Decline('number_range')
    return int(field)


def table(data):
    """What engine.BestHits holds for ``data``: {'n_lines', 'pass': [(off,
    len)], 'groups': [(key, first_line, best_line, score, off, len)] in
    first-seen order}.  Raises Decline(reason) at the first data line outside
    the native grammar: few fields, then field 0, then field 1."""
    passes, groups, index = [], [], {}
    off = 0
    lines = lines_of(data)
    for k, line in enumerate(lines):
        if line[:1] in PASS_BYTES:
            passes.append((off, len(line)))
        else:
            fields = line.split(b'\t')
            if len(fields) < 10:
                raise Decline('few_fields')
            score = _native_field(fields[0]) - _native_field(fields[1])
            key = fields[9]
            if key not in index:
                index[key] = len(groups)
                groups.append([key, k, k, score, off, len(line)])
            elif score > groups[index[key]][3]:
                groups[index[key]][2:] = [k, score, off, len(line)]
        off += len(line)
    return {'n_lines': len(lines), 'pass': passes, 'groups': [tuple(g) for g in groups]}


def native_path(data):
    """'native', or the reason the device path declines ``data`` with"""
    try:
        table(data)
    except Decline as d:
        return d.args[0]
    return 'native'


# ---------------------------------------------------------------------------
# PSL lines
# ---------------------------------------------------------------------------

def psl_line(matches, mismatches, qname, blocks=1, fields=21, end=b'\n', tname=b'chr1'):
    """One PSL data line: ``fields`` of the format's 21 columns, the block
    lists ``blocks`` entries long"""
    if isinstance(qname, str):
        qname = qname.encode('latin-1')
    num = lambda x: x if isinstance(x, bytes) else str(x).encode()  # noqa: E731
    sizes = b''.join(b'%d,' % (30 + j % 7) for j in range(blocks))
    starts = b''.join(b'%d,' % (1000 + 40 * j) for j in range(blocks))
    cols = [num(matches), num(mismatches), b'0', b'0', b'0', b'0', b'1', b'120', b'+', qname,
            b'350', b'0', b'340', tname, b'1500000', b'1000', b'1460', num(blocks), sizes, starts,
            starts]
    return b'\t'.join(cols[:fields]) + end


def cases():
    """name -> (text, 'native' or the reason the device path declines with)"""
    L = psl_line
    good = L(50, 2, 'q1') + L(40, 0, 'q2')
    c = {
        'header': (HEADER + b' \t \n' + L(10, 1, 'q1') + L(12, 1, 'q1') + b'\n' + L(5, 0, 'q2'),
                   'native'),
        'tie_first_wins': (L(10, 2, 'q1', tname=b'first') + L(9, 1, 'q1', tname=b'second') +
                           L(8, 0, 'q1', tname=b'third'), 'native'),
        'later_strictly_greater': (L(10, 2, 'q1', tname=b'a') + L(10, 1, 'q1', tname=b'b') +
                                   L(9, 0, 'q1', tname=b'c') + L(3, 0, 'q2'), 'native'),
        'negative_scores': (L(2, 9, 'q1', tname=b'a') + L(0, 3, 'q1', tname=b'b') +
                            L(0, INT_MAX, 'q2') + L(INT_MAX, 0, 'q3'), 'native'),
        'ten_fields': (L(5, 1, 'q1', fields=10) + L(9, 1, 'q1') + L(7, 1, 'q1', fields=10) +
                       L(3, 1, 'q1'), 'native'),
        'ten_fields_crlf': (L(5, 1, 'q1', fields=10, end=b'\r\n') + L(9, 1, 'q1', end=b'\r\n') +
                            L(7, 1, 'q1', fields=10, end=b'\r\n') + L(8, 1, 'q1', fields=10),
                            'native'),
        'empty_key': (L(5, 1, '') + L(6, 1, '') + L(1, 0, 'q') + L(4, 0, '', fields=10),
                      'native'),
        'case_and_space': (L(5, 1, 'Query') + L(6, 1, 'query') + L(7, 1, 'que ry') +
                           L(8, 1, 'query ') + L(9, 1, 'query'), 'native'),
        'key_lengths': (L(5, 1, 'x') + L(6, 1, 'k' * 300) + L(7, 1, 'x') + L(1, 1, 'k' * 300) +
                        L(2, 2, 'k' * 299 + 'j'), 'native'),
        'long_line': (L(5, 1, 'q1') + L(7, 1, 'q1', blocks=900) + L(6, 1, 'q2', blocks=900) +
                      L(9, 9, 'q2'), 'native'),
        'last_line_no_lf': (L(5, 1, 'q1') + L(7, 1, 'q1')[:-1], 'native'),
        'last_line_no_lf_ten_fields': (L(5, 1, 'q1', fields=10) + L(7, 1, 'q1', fields=10)[:-1],
                                       'native'),
        'last_line_no_lf_header': (L(5, 1, 'q1') + b'psl', 'native'),
        'empty_file': (b'', 'native'),
        'only_lfs': (b'\n\n\n', 'native'),
        'hash_line': (b'# a comment\n' + good, 'few_fields'),
        'few_fields_first': (L(5, 1, 'q1', fields=9) + good, 'few_fields'),
        'few_fields_after_good': (good + L(5, 1, 'q1', fields=9) + good, 'few_fields'),
        'few_fields_after_header': (HEADER + good + b'psl\n' + L(5, 1, 'q1', fields=3) +
                                    b'more\n' + good, 'few_fields'),
        'cr_lf_alone': (good + b'\r\n' + good, 'few_fields'),
        'field0_not_a_number': (good + L(b'x5', 1, 'q1'), 'integer_form'),
        'field1_empty': (good + L(b'1', b'', 'q1') + good, 'integer_form'),
        'plus_sign': (good + L(b'+5', 1, 'q1') + L(90, 0, 'q2'), 'integer_form'),
        'blank_in_field1': (good + L(9, b' 7', 'q1') + L(90, 0, 'q2'), 'integer_form'),
        'blanks_around': (L(b'7 ', b'\x0b1\x0c', 'q1') + good, 'integer_form'),
        # field 0 cannot carry the sign: a line that starts with '-' is a pass-through line
        'minus_sign': (good + L(3, b'-3', 'q1') + L(1, b'-30', 'q2'), 'integer_form'),
        'minus_first_byte': (good + L(b'-3', 1, 'q1') + L(b' 7', 1, 'q1'), 'native'),
        'underscore': (HEADER + good + L(b'1_0', 1, 'q1') + good, 'integer_form'),
        'eleven_digits': (good + L(b'00000000012', 1, 'q1') + L(2, b'12345678901', 'q3'),
                          'number_range'),
        'two_to_the_31': (good + L(1, 2147483648, 'q1') + L(2147483648, 0, 'q9'), 'number_range'),
        'ten_digits_in_range': (L(b'0000000012', b'2147483647', 'q1') + L(b'2147483647', 0, 'q1'),
                                'native'),
    }
    for seed in range(6):  # the last two with one line outside the grammar
        text = random_text(20261100 + seed, bad=seed >= 4)
        c['random_%d' % seed] = (text, native_path(text))
    return c


def random_text(seed, bad=False):
    """A few dozen lines: header lines anywhere, a few keys, small scores;
    ``bad``: one line outside the native grammar among them"""
    rnd = random.Random(seed)
    keys = ['q%d' % rnd.randrange(40) for _ in range(rnd.randrange(1, 9))] + ['Q 1', '']
    parts = [HEADER] if rnd.random() < 0.5 else []
    for _ in range(rnd.randrange(1, 40)):
        r = rnd.random()
        if r < 0.08:
            parts.append(rnd.choice([b'\n', b'   \n', b'\t\n', b'--\n', b'match\n', b'psl\n']))
        else:
            parts.append(psl_line(rnd.randrange(12), rnd.randrange(12), rnd.choice(keys),
                                  blocks=rnd.randrange(1, 5),
                                  fields=10 if rnd.random() < 0.15 else 21,
                                  end=b'\r\n' if rnd.random() < 0.1 else b'\n'))
    if bad:
        parts.insert(rnd.randrange(len(parts) + 1),
                     rnd.choice([psl_line(3, 1, 'q1', fields=rnd.randrange(1, 10)),
                                 psl_line(b'+5', 1, 'q1'), psl_line(4, b'12345678901', 'q1')]))
    text = b''.join(parts)
    return text[:-1] if rnd.random() < 0.3 else text


# ---------------------------------------------------------------------------
# the device tests' worlds
# ---------------------------------------------------------------------------

SIZES = (0, 1, 63, 64, 65, 255, 256, 257, 4099)
SHAPES = ('one', 'distinct', 'mix')


def world(n_data, shape, seed=20261020):
    """A PSL text of ``n_data`` data lines.  Its first line is a pass-through
    line of exactly TEXT_BLOCK bytes, so its LF is the last byte of a text
    block and the next line starts at a block's first byte; one line is longer
    than 8192 bytes (the middle data line; a pass-through line when there is
    none); three header lines stand in the middle.  ``shape``: 'one' key for
    all lines, all keys 'distinct', or a heavy-tailed 'mix' with ties, 10-field
    lines, negative scores, and a key whose last line is its best."""
    rnd = random.Random(seed * 31 + n_data * 3 + SHAPES.index(shape))
    lines = []
    for k in range(n_data):
        if shape == 'one':
            key, fields = 'the_only_query', 21
        elif shape == 'distinct':
            key, fields = 'q%d_%d' % (k, rnd.randrange(1000)), 21
        else:
            key = 'q%d' % min(int(rnd.paretovariate(0.7)), max(n_data // 3, 1))
            fields = 10 if rnd.random() < 0.1 else 21
        m, mm = rnd.randrange(3), rnd.randrange(3)  # five scores: ties at the top of most keys
        blocks = 1200 if k == n_data // 2 else rnd.randrange(1, 4)
        if blocks == 1200:
            fields = 21  # the long line carries its block lists
        lines.append(psl_line(m, mm, key, blocks=blocks, fields=fields))
    if shape == 'mix' and n_data >= 63:  # a key whose last line is its best
        lines[-1] = psl_line(1000, 0, 'q1')
    if not n_data:
        lines.append(b'p' + b'x' * 9000 + b'\n')
    mid = len(lines) // 2
    lines[mid:mid] = [b'\n', b'match\tmis-\n', b'-----\n']
    first = b'psLayout version 3 ' + b'.' * TEXT_BLOCK
    return first[:TEXT_BLOCK - 1] + b'\n' + b''.join(lines)
