"""replace_names on the device (rename.hip; genome_tools.py:431-446):
engine.NameReplacer against the field model of replace_expect.py -- hits and
output, exactly -- on seeded texts of many text blocks with names at, before,
behind and across every block edge; fields around the longest name and of a
megabyte; a narrowed hash with thousands of false hits, and a clash; copies of
every source and destination misalignment; both rank orders; the declines; and
every run recorded from the reference through the class and the tool on both
paths.  The shapes derive from NameReplacer.params()."""

import os
import random
import subprocess
import sys

import numpy as np
import pytest

import replace_expect as rx
from magot_amd import engine, genome_tools

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = rx.load()
NAMES = sorted(GOLD)
NATIVE = [(n, o) for n in NAMES for o in rx.ORDERS if GOLD[n]['path'][o] == 'native']
HOST = [(n, o) for n in NAMES for o in rx.ORDERS
        if GOLD[n]['path'][o] not in ('native', 'IndexError')]
PARAMS = engine.NameReplacer.params()
BLOCK, MAX_NAME, PIECE = PARAMS['text_block'], PARAMS['max_name'], PARAMS['piece']
D = b';'
LOWER = b'abcdefghijklmnopqrstuvwxyz'
_cache = {}


def b(text):
    return text.encode('latin-1')


def _native(text, names, values, d=D, ranks=None, **kw):
    """engine.NameReplacer of a call that must not be declined"""
    rep = engine.NameReplacer.parse(text, names, values, d, ranks, **kw)
    assert isinstance(rep, engine.NameReplacer), rep
    return rep


def _assert_equals_model(text, names, values, d=D, ranks=None, **kw):
    """hits, sizes and output of the device are the field model's"""
    ranks = list(range(len(names))) if ranks is None else list(ranks)
    want, hits = rx.field_model(text, names, values, ranks, d)
    rep = _native(text, names, values, d, ranks, **kw)
    try:
        assert rep.n_fields == text.count(d)
        assert rep.n_lines == len(rx.lines_of(text))
        assert (rep.n_hits, rep.out_bytes) == (len(hits), len(want))
        got = rep.hits()
        assert (got['end'].dtype, got['key'].dtype) == (np.uint64, np.uint32)
        assert list(zip(got['end'].tolist(), got['key'].tolist())) == hits
        assert rep.render().tobytes() == want
    finally:
        rep.close()
    return hits


def table():
    """8 lowercase names of every length from 1 to max_name, values in upper
    case and digits (no name is a suffix of one, none is a suffix of a name),
    shorter, as long and longer than their names; once"""
    if 'table' not in _cache:
        rnd = random.Random(431)
        names = {}
        for size in range(1, MAX_NAME + 1):
            have = 0
            while have < (8 if size > 1 else 5):
                n = bytes(rnd.choice(LOWER[:6]) for _ in range(size))
                if n not in names:
                    names[n] = bytes(rnd.choice(b'ABCDEFGH0123456789')
                                     for _ in range(rnd.choice([1, size, size + 5, 40])))
                    have += 1
        names = list(names.items())
        rnd.shuffle(names)
        _cache['table'] = ([n for n, _ in names], [v for _, v in names])
    return _cache['table']


def filler(rnd, size):
    """fields of the names' alphabet and others, some of them names, in lines"""
    names, _ = table()
    out = bytearray()
    while len(out) < size:
        r = rnd.random()
        if r < 0.3:
            out += rnd.choice(names)[:40]
        elif r < 0.6:
            out += bytes(rnd.choice(LOWER[:6]) for _ in range(rnd.randint(0, 3)))
        else:
            out += bytes(rnd.choice(LOWER) for _ in range(rnd.randint(0, 12)))
        out += b'\n' if rnd.random() < 0.1 else D
    return out[:size]


def place(text, name, d_at):
    """`name` and its delimiter written into the text, the delimiter at d_at"""
    start = d_at - len(name)
    text[start - 1:d_at + 1] = D + name + D
    return d_at


@pytest.mark.parametrize('where', ['at', 'before', 'behind', 'across'])
def test_names_at_every_block_edge(where):
    """A text of 21 text blocks.  'at': at every edge a name whose delimiter is
    the block's last byte; 'before', 'behind': one byte to either side;
    'across': a name of 17 bytes with 1 to 16 of them before the edge, and one
    of max_name bytes with 1, half and all but one before it."""
    names, values = table()
    rnd = random.Random(len(where))
    text = filler(rnd, 21 * BLOCK)
    by_len = {}
    for n in names:
        by_len.setdefault(len(n), n)
    placed = []
    for k in range(1, 21):
        edge = k * BLOCK
        if where == 'across':
            name = by_len[17] if k <= 16 else by_len[MAX_NAME]
            before = k if k <= 16 else {17: 1, 18: MAX_NAME // 2, 19: MAX_NAME - 1, 20: 2}[k]
            placed.append(place(text, name, edge - before + len(name)))
        else:
            name = by_len[1 + (37 * k) % MAX_NAME]
            placed.append(place(text, name, edge - 1 + {'before': -1, 'at': 0, 'behind': 1}[where]))
    text = bytes(text)
    hits = _assert_equals_model(text, names, values)
    assert set(placed) <= {end for end, _ in hits}
    assert len(hits) > 1000 and len({len(names[k]) for _, k in hits}) > 30


def test_fields_around_the_longest_name_and_of_a_megabyte():
    rnd = random.Random(7)
    word = lambda size: bytes(rnd.choice(LOWER) for _ in range(size))
    longest, shorter, short = word(MAX_NAME), word(MAX_NAME - 1), b'zq'
    names, values = [longest, shorter, short], [b'LONGEST', b'SHORTER', b'S' * 300]
    fields = [shorter, b'X' + shorter, b'XY' + shorter, longest, b'X' + longest,
              b'X' * 700 + longest, b'X' * (MAX_NAME - 3) + short, b'X' * (MAX_NAME - 2) + short,
              b'X' * (MAX_NAME - 1) + short, longest[1:], shorter[1:]]
    text = D.join(fields) + D + b'\n'
    hits = _assert_equals_model(text, names, values)
    assert len(hits) == len(fields) - 2
    mega = 1 << 20
    # one field of a megabyte, and one line of a megabyte of short fields
    text = b'X' * mega + longest + D + b'\n' + (b'abc' + D) * (mega // 4) + short + D
    hits = _assert_equals_model(text, names, values)
    assert [k for _, k in hits] == [0, 2]


def hashed_names(bits, count, clash):
    """names of distinct low `bits` bits of the matching hash; with `clash` the
    last one shares its bucket with the first"""
    rnd = random.Random(bits)
    seen, names = {}, []
    while len(names) < count:
        n = bytes(rnd.choice(LOWER[:4]) for _ in range(rnd.randint(1, 6)))
        h = rx.match_hash(n, bits)
        if h not in seen:
            seen[h] = n
            names.append(n)
    while clash:
        n = bytes(rnd.choice(LOWER[:4]) for _ in range(rnd.randint(1, 6)))
        if n not in names and rx.match_hash(n, bits) == rx.match_hash(names[0], bits):
            return names + [n]
    return names


def test_a_narrow_hash_rejects_its_false_hits():
    names = hashed_names(8, 200, False)
    values = [b'<%d>' % k for k in range(len(names))]
    rnd = random.Random(8)
    text = b''.join(bytes(rnd.choice(LOWER[:4]) for _ in range(rnd.randint(0, 7))) +
                    (b'\n' if rnd.random() < 0.05 else D) for _ in range(6000))
    listed = set(names)
    false_hits = sum(1 for f in text.replace(b'\n', D).split(D)
                     for size in range(1, len(f) + 1)
                     if f[len(f) - size:] not in listed)
    assert false_hits > 5000  # 200 of 256 buckets are taken: most of them meet a name's hash
    hits = _assert_equals_model(text, names, values, hash_bits=8)
    assert len(hits) > 500
    assert _assert_equals_model(text, names, values) == hits


def test_a_clash_declines_and_hash_bits_are_checked():
    names = hashed_names(8, 100, True)
    values = [b'V'] * len(names)
    assert engine.NameReplacer.parse(b'a;b;\n', names, values, D, hash_bits=8) == \
        (None, 'hash_collision')
    rep = _native(b'a;b;\n', names, values)  # all 64 bits tell them apart
    rep.close()
    rep = _native(b'a;b;\n', names[:1], values[:1], hash_bits=1)  # one name clashes with nothing
    rep.close()
    for bits in (0, 65):
        with pytest.raises(engine.MagotError, match='hash_bits'):
            engine.NameReplacer.parse(b'a;\n', [b'a'], [b'A'], D, hash_bits=bits)
    with pytest.raises(engine.MagotError, match='delimiter'):
        engine.NameReplacer.parse(b'a\n', [b'a'], [b'A'], b'\n')
    for bad in ([b''], [b'n' * (MAX_NAME + 1)]):
        with pytest.raises(engine.MagotError, match='name'):
            engine.NameReplacer.parse(b'a;\n', bad, [b'A'], D)
    with pytest.raises(engine.MagotError, match='rank'):
        engine.NameReplacer.parse(b'a;\n', [b'a'], [b'A'], D, ranks=[1])


def test_copies_of_every_misalignment():
    """Replacements that shrink, keep and grow: unchanged runs of 0 to 40 bytes
    and of a piece and more between hits whose values have every length from 0
    to 33, so that run and value pieces meet all 16 x 16 pairs of source and
    destination misalignment; the text spans several blocks and pieces."""
    rnd = random.Random(16)
    names = [b'k%02d' % k for k in range(34)]
    values = [bytes(rnd.choice(b'ABCDEFGH') for _ in range(k)) for k in range(34)]
    ranks = list(range(34))
    ranks[0], ranks[33] = 33, 0  # the empty value in the last rank
    parts = []
    for i in range(1500):
        run = rnd.choice([0, rnd.randint(0, 40), rnd.randint(0, 40), PIECE + rnd.randint(-20, 20)]
                         if i % 50 else [2 * PIECE + 5])
        parts.append(b'.' * run + rnd.choice(names) + D)
    text = b''.join(parts) + b'tail'
    want, hits = rx.field_model(text, names, values, ranks, D)
    # the pairs (source, destination) mod 16 of the unchanged runs and of the values
    pairs, shift, prev = set(), 0, 0
    blob_at = np.cumsum([0] + [len(v) for v in values])
    for end, k in hits:
        start = end - len(names[k])
        pairs.add((prev % 16, (prev + shift) % 16))
        pairs.add((int(blob_at[k]) % 16, (start + shift) % 16))
        shift += len(values[k]) - len(names[k])
        prev = end
    assert len(pairs) == 256
    assert len(text) > 3 * BLOCK and len(want) != len(text)
    assert _assert_equals_model(text, names, values, ranks=ranks) == hits


@pytest.mark.parametrize('order', rx.ORDERS)
def test_rank_order_and_the_last_value(order, tmp_path, capfdbinary):
    """three nested names end at one delimiter: the dict's first wins; a
    repeated row's last value is printed"""
    case = GOLD['nested_semicolon']
    text, tab, d = b(case['text']), b(case['table']) + b'11\tLAST\tx\n', b(case['name_end'])
    names, values = rx.keyed(rx.table_rows(tab))
    ranks = rx.ranks_of(names, d, order)
    assert values[names.index(b'11')] == b'LAST'
    hits = _assert_equals_model(text, names, values, d, ranks)
    first = {k: r for k, r in zip(range(3), ranks)}
    assert hits[0] == (3, min(first, key=first.get))  # the field 111
    want, _ = rx.expected_loop(text, tab, d, order)
    path, table_path = str(tmp_path / 't.txt'), str(tmp_path / 'n.tsv')
    with open(path, 'wb') as fh:
        fh.write(text)
    with open(table_path, 'wb') as fh:
        fh.write(tab)
    genome_tools.replace_names(path, table_path, ';', order=order)
    assert capfdbinary.readouterr().out == want
    assert genome_tools.replace_names.last_path == ('replace_names', 'native', None)


def test_declines_and_empty_inputs():
    names, values = table()
    text = bytes(filler(random.Random(3), 3 * BLOCK))
    assert engine.NameReplacer.parse(text, names, values, D, max_bytes=len(text) - 1) == \
        (None, 'too_large')
    assert engine.NameReplacer.parse(text, names, values, D, max_bytes=1) == (None, 'too_large')
    _assert_equals_model(text, names, values, max_bytes=len(text))
    _assert_equals_model(b'', names, values)
    _assert_equals_model(text, [], [])
    _assert_equals_model(b'', [], [])
    _assert_equals_model(b';', [b'x'], [b'X'])
    _assert_equals_model(b'x;', [b'x'], [b''])
    rep = _native(text, names, values)
    try:
        want = rep.render().tobytes()
        t = rep.time(1)
        assert set(t) == set(engine.NameReplacer.PASSES) | {'text_bytes', 'out_bytes'}
        assert (t['text_bytes'], t['out_bytes']) == (len(text), len(want))
        assert all(t[p] > 0 for p in engine.NameReplacer.PASSES)
        assert rep.render().tobytes() == want  # the answers stand
    finally:
        rep.close()


def _call(fn, capfdbinary, *args, **kw):
    exc = None
    try:
        fn(*args, **kw)
    except Exception as e:  # noqa: BLE001
        exc = type(e).__name__
    return capfdbinary.readouterr().out.decode('latin-1'), exc


def write_case(tmp_path, case):
    path, table_path = str(tmp_path / 'text.txt'), str(tmp_path / 'names.tsv')
    with open(path, 'wb') as fh:
        fh.write(b(case['text']))
    with open(table_path, 'wb') as fh:
        fh.write(b(case['table']))
    return path, table_path


@pytest.mark.parametrize('name,order', NATIVE, ids=['%s-%s' % c for c in NATIVE])
def test_native_goldens_through_the_class_and_the_tool(name, order, tmp_path, capfdbinary):
    case = GOLD[name]
    text, tab, d = b(case['text']), b(case['table']), b(case['name_end'])
    want = case['out_py2'] if order == 'py2' else case['out']
    names, values = rx.keyed(rx.table_rows(tab))
    rep = _native(text, names, values, d, rx.ranks_of(names, d, order))
    try:
        assert rep.render().tobytes().decode('latin-1') == want
    finally:
        rep.close()
    path, table_path = write_case(tmp_path, case)
    got = _call(genome_tools.replace_names, capfdbinary, path, table_path, case['name_end'],
                order=order)
    assert got == (want, None)
    assert genome_tools.replace_names.last_path == ('replace_names', 'native', None)


@pytest.mark.parametrize('name,order', HOST, ids=['%s-%s' % c for c in HOST])
def test_host_goldens_through_the_tool_name_their_decline(name, order, tmp_path, capfdbinary):
    case = GOLD[name]
    path, table_path = write_case(tmp_path, case)
    got = _call(genome_tools.replace_names, capfdbinary, path, table_path, case['name_end'],
                order=order)
    assert got == (case['out_py2'] if order == 'py2' else case['out'], None)
    assert genome_tools.replace_names.last_path == ('replace_names', 'host', case['path'][order])


def test_a_tabless_table_raises_before_any_output(tmp_path, capfdbinary):
    for name in ('tabless_line', 'tabless_last_line'):
        path, table_path = write_case(tmp_path, GOLD[name])
        assert _call(genome_tools.replace_names, capfdbinary, path, table_path) == \
            ('', 'IndexError')


def test_the_command_line_prints_the_references_bytes(tmp_path):
    case = GOLD['gff_ids']
    path, table_path = write_case(tmp_path, case)
    env = dict(os.environ, PYTHONPATH=ROOT)
    argv = [sys.executable, '-m', 'magot_amd.genome_tools', 'replace_names', path, table_path,
            'name_end=;']
    res = subprocess.run(argv, stdout=subprocess.PIPE, stderr=subprocess.PIPE, env=env, timeout=300)
    assert res.returncode == 0, res.stderr[-2000:]
    assert res.stdout == b(case['out_py2'])
