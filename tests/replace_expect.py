"""What replace_names (genome_tools.py:431-446) prints, restated twice for the
tests: the reference's loop over the keys, and the field model the device path
rests on -- a line is its fields (what lies between two delimiters), and a
field is rewritten at most once, by the key of lowest rank whose name is a
suffix of it.  Also the cases recorded in tests/golden/replace.json, the
decision whether the field model is exact for a table (with all pairs of keys
compared, where genome_tools probes sets), the matching hash of rename.hip and
seeded worlds for the device tests.  Nothing here imports the code under
test."""

import json
import os
import random

from magot_amd import py2order

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, 'golden')

ORDERS = ('insertion', 'py2')
# what the host tests assume where no device is asked (test_gpu_replace.py reads
# engine.NameReplacer.params())
PARAMS = {'max_name': 256, 'text_block': 4096, 'piece': 4096}


def load():
    with open(os.path.join(GOLDEN, 'replace.json')) as fh:
        return json.load(fh)


def lines_of(data):
    """``for line in open(path)`` of Python 2: lines end after LF only"""
    parts = data.split(b'\n')
    last = parts.pop()
    return [p + b'\n' for p in parts] + ([last] if last else [])


def table_rows(table):
    """[(name, f1)] of a table's lines; IndexError for a line without a TAB"""
    rows = []
    for line in lines_of(table):
        fields = line.split(b'\t')
        rows.append((fields[0], fields[1]))
    return rows


def keyed(rows):
    """(names first seen, the last value of each)"""
    table = {}
    for name, f1 in rows:
        table[name] = f1
    return list(table), list(table.values())


def dict_order(names, name_end, order):
    """the indices of ``names`` in the order the dict of name + name_end iterates"""
    if order == 'insertion':
        return list(range(len(names)))
    keys = [(n + name_end).decode('latin-1') for n in names]
    at = {k: i for i, k in enumerate(keys)}
    return [at[k] for k in py2order.dict_order(keys)]


def expected_loop(text, table, name_end, order):
    """(stdout, exception name) of the reference's loop"""
    try:
        names, values = keyed(table_rows(table))
    except IndexError:
        return b'', 'IndexError'
    pairs = [(names[i] + name_end, values[i] + name_end)
             for i in dict_order(names, name_end, order)]
    out = []
    for line in lines_of(text):
        for word, new in pairs:
            if word in line:
                line = line.replace(word, new)
        out.append(line[:-1] + b'\n')
    return b''.join(out), None


def field_model(text, names, values, ranks, d):
    """(what is printed, [(the offset of the field's delimiter, the key)] in
    text order): of the names that are suffixes of a field the one of lowest
    rank gives way to its value; the text's last byte gives way to an LF"""
    by_name = {n: k for k, n in enumerate(names)}
    longest = max([len(n) for n in names] or [0])
    out, hits, at = [], [], 0
    for line in text.split(b'\n'):
        parts = line.split(d)
        pos = at
        for i, part in enumerate(parts[:-1]):
            end = pos + len(part)
            best = None
            for size in range(1, min(len(part), longest) + 1):
                k = by_name.get(part[len(part) - size:])
                if k is not None and (best is None or ranks[k] < ranks[best]):
                    best = k
            if best is not None:
                parts[i] = part[:len(part) - len(names[best])] + values[best]
                hits.append((end, best))
            pos = end + 1
        out.append(d.join(parts))
        at += len(line) + 1
    whole = b'\n'.join(out)
    return (whole[:-1] + b'\n' if whole else b''), hits


def ranks_of(names, name_end, order):
    ranks = [0] * len(names)
    for r, i in enumerate(dict_order(names, name_end, order)):
        ranks[i] = r
    return ranks


def expected_fields(text, table, name_end, order):
    """the field model's output for a table inside its conditions"""
    names, values = keyed(table_rows(table))
    return field_model(text, names, values, ranks_of(names, name_end, order), name_end)[0]


def note(table, name_end, order, params=PARAMS):
    """'native' where the field model is exact for the table, 'IndexError'
    where the table raises, else the reason the host loop is taken for, in the
    order genome_tools.replace_names decides"""
    try:
        names, values = keyed(table_rows(table))
    except IndexError:
        return 'IndexError'
    if len(name_end) != 1 or name_end == b'\n':
        return 'name_end'
    if any(not n for n in names):
        return 'empty_name'
    if any(len(n) > params['max_name'] for n in names):
        return 'long_name'
    if any(name_end in n for n in names):
        return 'delimiter_in_name'
    if any(name_end in v for v in values):
        return 'delimiter_in_value'
    seq = dict_order(names, name_end, order)
    for a, i in enumerate(seq):  # all pairs: the tables here are small
        for j in seq[a + 1:]:
            if values[i].endswith(names[j]) or \
                    (names[j].endswith(values[i]) and len(values[i]) < len(names[j])):
                return 'chain'
    return 'native'


def notes(case, params=PARAMS):
    return {order: note(case['table'], case['name_end'], order, params) for order in ORDERS}


def cases():
    """name -> {'text': bytes, 'table': bytes, 'name_end': bytes}"""
    def case(text, table, name_end=b' '):
        return {'text': text, 'table': table, 'name_end': name_end}

    gff = (b'chr1\tsrc\tgene\t1\t9\t.\t+\t.\tID=g1;Name=g11;Note=xg1;\n'
           b'chr1\tsrc\tmRNA\t1\t9\t.\t+\t.\tID=g1.t1;Parent=g1;\n'
           b'g1;g1;;g111;ID=g2\n')
    nested = b'11\tBB\tx\n111\tCCC\tx\n1\tA\tx\n'
    return {
        'issue_two_fields': case(b'gene1 gene2 gene10 x\ngene2 \n', b'gene1\tG1\ngene2\tG2\n'),
        'three_fields': case(b'gene1 gene2 gene10 x\ngene2 \n', b'gene1\tG1\tx\ngene2\tG2\ty\n'),
        'trailing_tab': case(b'a b c \nb a\n', b'a\tAA\t\nb\t\t\n'),
        'crlf_table': case(b'a b c \r\nb a \r\n', b'a\tAA\r\nb\tBB\tz\r\n'),
        'last_row_without_lf': case(b'a b c \nb a \n', b'a\tAA\tx\nb\tBB'),
        'last_row_three_fields_without_lf': case(b'a b c \nb a \n', b'a\tAA\tx\nb\tBB\ty'),
        'repeated_name': case(b'a b a \n', b'a\tfirst\tx\nb\tB\tx\na\tlast\tx\n'),
        'nested_semicolon': case(b'111;11;1;2111;x1;21;\n;1;;111\n', nested, b';'),
        'nested_space': case(b'111 11 1 2111 x1 21 \n 1  111\n', nested),
        'nested_tab': case(b'111\t11\t1\t2111\tx1\t21\t\n\t1\t\t111\n', nested, b'\t'),
        'nested_many': case(b''.join(b'%d;' % i for i in range(1200)) + b'\n',
                            b''.join(b'%d\t<%d>\tx\n' % (i, i) for i in range(0, 1200, 7)), b';'),
        'suffix_of_a_word': case(b'xgene1;gene1x;agene1;\n', b'gene1\tG\tx\n', b';'),
        'whole_field': case(b';gene1;gene1;;gene1\n', b'gene1\tG\tx\n', b';'),
        'offset_zero': case(b'gene1;rest\ngene1;\n', b'gene1\tLONGER\tx\n', b';'),
        'gff_ids': case(gff, b'g1\tGENE0001\tx\ng1.t1\tGENE0001.1\tx\ng2\tGENE0002\tx\n', b';'),
        'high_byte_and_cr': case(b'\xe9t\xe9;a\rb;\xff;\r;\r\n\xe9;b;\n',
                                 b'\xe9\tE\tx\na\rb\t\xfe\r\tx\n\xff\t\xff\xff\tx\n\r\tCR\tx\n', b';'),
        'empty_value_last_rank': case(b'ab;b;cab;\n', b'ab\t\tx\n', b';'),
        'empty_value_earlier': case(b'ab;b;cab;\n', b'ab\t\tx\nb\tB\tx\nq\tQ\tx\n', b';'),
        'chain_forward': case(b'a;b;c;xa;\n', b'a\tb\tx\nb\tc\tx\n', b';'),
        'chain_backward': case(b'a;b;c;xa;\n', b'b\tc\tx\na\tb\tx\n', b';'),
        'chain_by_suffix': case(b'xa;a;ya;\n', b'a\ty\tx\nxy\tZ\tx\n', b';'),
        'value_with_delimiter': case(b'a;b;\n', b'a\tb;b\tx\nb\tc\tx\n', b';'),
        'name_with_delimiter': case(b'a;b;a;\n', b'a;b\tX\tx\nb\tY\tx\n', b';'),
        'name_end_empty': case(b'abc abc\nb\n', b'b\tBB\tx\nc\tb\tx\n', b''),
        'name_end_two_bytes': case(b'a, b, a,b\n', b'a\tA\tx\nb\tB\tx\n', b', '),
        'empty_name': case(b'a b  c\n', b'\tE\tx\na\tA\tx\n'),
        'tabless_line': case(b'a b\n', b'a\tA\tx\nno tab here\nb\tB\tx\n'),
        'tabless_last_line': case(b'a b\n', b'a\tA\tx\nb'),
        'empty_table': case(b'a b \nc\n', b''),
        'empty_text': case(b'', b'a\tA\tx\n'),
        'both_empty': case(b'', b''),
        'no_final_lf_name_and_d': case(b'x y\nz gene1;', b'gene1\tG1\tx\n', b';'),
        'no_final_lf_two_fields': case(b'gene1;gene1;', b'gene1\tG1\n', b';'),
        'no_final_lf_plain': case(b'gene1;gene', b'gene1\tG1\tx\n', b';'),
        'one_byte_text': case(b'x', b'x\tX\tx\n'),
        'one_byte_delimiter': case(b';', b'x\tX\tx\n', b';'),
        'one_byte_lf': case(b'\n', b'x\tX\tx\n'),
        'blank_lines': case(b'\n\na \n\n', b'a\tA\tx\n'),
        'shrink_keep_grow': case(b'long1;same;s;long1;s;same;\n' * 3,
                                 b'long1\tl\tx\nsame\tSAME\tx\ns\tSSSSSSSSSSSSSSSSSSSSS\tx\n', b';'),
        'long_name': case(b'x;' + b'n' * 300 + b';\n', b'n' * 300 + b'\tN\tx\n', b';'),
    }


# ---------------------------------------------------------------------------
# rename.hip's matching hash, for the tests that choose names by their bucket
# ---------------------------------------------------------------------------
_MASK64 = (1 << 64) - 1


def match_hash(name, bits=64):
    """from the name's last byte to its first, masked to ``bits``"""
    h = 0xcbf29ce484222325
    for c in reversed(name):
        h = ((h ^ c) * 0x100000001b3) & _MASK64
    return h & ((1 << bits) - 1)


def fuzz_case(rnd):
    """a small random (text, table, name_end): nested names, values that are
    names, empty values, CRs, two- and three-field rows"""
    d = rnd.choice([b' ', b';', b'\t', b'a'])
    alphabet = rnd.choice([b'ab', b'abc', b'ab\r', b'01' + d, b'xy' + d])
    word = lambda lo, hi: bytes(rnd.choice(alphabet) for _ in range(rnd.randint(lo, hi)))
    rows = []
    for _ in range(rnd.randint(0, 4)):
        name = word(1, 3).replace(b'\t', b'')
        value = rnd.choice([word(0, 3), word(1, 2) + b'!', b'']).replace(b'\t', b'')
        shape = rnd.randint(0, 2)
        rows.append(name + b'\t' + value + (b'\n', b'\tx\n', b'\t\n')[shape])
    text = b''
    for _ in range(rnd.randint(0, 3)):
        for _ in range(rnd.randint(0, 5)):
            text += word(0, 4) + (d if rnd.random() < 0.8 else b'')
        text += b'\n'
    if text and rnd.random() < 0.3:
        text = text[:-1]
    return text, b''.join(rows), d
