"""exclude_from_fasta and fasta2tab on the device (fastarec.hip;
genome_tools.py:377-391, magot_smallfuncs.py:21-29): engine.FastaRecords against
the restated tables of fasta_expect.py on seeded worlds, exactly; the membership
under full and narrowed hashes; the reflow byte for byte in both styles and
orders; every decline with its line; every run recorded from the reference
through both tools on both paths; one command-line call.

Worlds: 0, 1, around a wave and around a workgroup of records, and 4099 (the
sort and the line index then span several blocks), each with all names
distinct, one name for all records, and a mix with repeats, empty records and
records of many lines.  Their line shapes derive from FastaRecords.params()."""

import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

import fasta_expect as fe
from magot_amd import engine, genome_tools, py2order

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = fe.load()
NAMES = sorted(GOLD)
WORLDS = [(n, shape) for n in fe.SIZES for shape in fe.SHAPES]
PARAMS = engine.FastaRecords.params()
_cache = {}


def world(n, shape):
    """(text, restated table) of a world, computed once"""
    if (n, shape) not in _cache:
        text = fe.world(n, shape, PARAMS)
        _cache[n, shape] = (text, fe.with_lines(fe.table(text, PARAMS), text))
    return _cache[n, shape]


def b(text):
    return text.encode('latin-1')


def _native(text, **kw):
    """engine.FastaRecords of a text that must not be declined"""
    recs = engine.FastaRecords.parse(text, **kw)
    assert isinstance(recs, engine.FastaRecords), (recs, engine.FastaRecords.declined_line)
    return recs


def _assert_equals_table(recs, want):
    assert recs.n_lines == want['n_lines']
    assert recs.n_records == len(want['records']) and recs.n_keys == len(want['keys'])
    assert recs.n_with_sequence == sum(1 for r in want['records'] if r[3])
    got = recs.records()
    for name, dtype in engine.FastaRecords.RECORD_COLUMNS:
        assert got[name].dtype == dtype and len(got[name]) == len(want['records'])
    cols = ('line', 'name_off', 'name_len', 'seq_len')
    assert list(zip(*[got[c].tolist() for c in cols])) == [r[:4] for r in want['records']]
    assert got['hash'].tolist() == [fe.str_hash(r[4]) for r in want['records']]
    cols = ('word_off', 'word_len')
    assert list(zip(*[got[c].tolist() for c in cols])) == [r[5:7] for r in want['records']]
    assert got['word_hash'].tolist() == [fe.str_hash(r[7]) for r in want['records']]
    assert got['no_word'].tolist() == [r[8] for r in want['records']]
    keys = recs.keys()
    for name, dtype in engine.FastaRecords.KEY_COLUMNS:
        assert keys[name].dtype == dtype and len(keys[name]) == len(want['keys'])
    cols = ('first_record', 'last_record', 'no_word')
    assert list(zip(*[keys[c].tolist() for c in cols])) == [k[1:] for k in want['keys']]
    assert keys['hash'].tolist() == [fe.str_hash(k[0]) for k in want['keys']]


def test_the_params_are_what_the_restatement_assumes():
    assert PARAMS == fe.PARAMS
    assert PARAMS['piece'] & (PARAMS['piece'] - 1) == 0


@pytest.mark.parametrize('n,shape', WORLDS, ids=['%d-%s' % w for w in WORLDS])
def test_tables_equal_the_restated_table(n, shape):
    text, want = world(n, shape)
    assert want['verdict'] is None and len(want['records']) == n
    recs = _native(text)
    try:
        _assert_equals_table(recs, want)
    finally:
        recs.close()


def test_the_worlds_hold_what_they_promise():
    P, B = PARAMS['piece'], PARAMS['text_block']
    for n, shape in WORLDS:
        if not n:
            assert world(n, shape)[0] == b''
            continue
        text, t = world(n, shape)
        lines = t['lines']
        assert not text.endswith(b'\n')  # a final line without an LF
        assert any((off + len(ln)) % B == 0 and ln.endswith(b'\n') for off, ln in lines[:-1])
        assert any(ln.endswith(b'\r\n') and (off + len(ln) - 1) % B == 0 for off, ln in lines)
        assert any(ln.endswith(b'\r\n') for _, ln in lines)
        assert any(ln.endswith(b'\n') and not ln.endswith(b'\r\n') for _, ln in lines)
        pay = [len(fe._payload(ln)) for _, ln in lines if ln[:1] != b'>']
        assert P in pay and P + 1 in pay and max(pay) > 3 * P
        keys = t['keys']
        if shape == 'one':
            assert len(keys) == 1 and keys[0][1:3] == (0, n - 1)
        if shape == 'distinct':
            assert len(keys) == n and all(k[1] == k[2] for k in keys)
        if n < 63:
            continue
        assert any(off % B == 0 and off and ln[:1] == b'>' for off, ln in lines)
        rec1 = [ln for _, ln in lines[t['records'][1][0] + 1:t['records'][2][0]]]
        assert len(rec1) >= 3 and all(len(fe._payload(ln)) == 1 for ln in rec1)
        if shape == 'one':
            continue
        if n >= 255:
            assert {r[2] for r in t['records']} >= set(range(1, 41))
        # every source and destination phase of a vector store, in either style
        for style in ('fasta', 'tab'):
            pairs = set()
            for src, dst, length in fe.pieces(t, range(n), style, P):
                first = (dst + 15) & ~15
                if first + 16 <= dst + length:
                    pairs.add((src & 15, dst & 15))
            if n >= 4099:  # some 10,000 pieces with a whole chunk
                assert len(pairs) == 256, (n, shape, style)
        if shape != 'mix' or n < 255:
            continue
        assert 1 < len(keys) < n
        assert any(not r[3] for r in t['records'])                       # empty records
        assert any(k[1] != k[2] for k in keys)                            # repeats
        first_of = {}
        for r, rec in enumerate(t['records']):
            first_of.setdefault(rec[4], r)
        assert any(first_of[k[0]] < k[1] for k in keys)  # a first occurrence without a sequence
        assert any(k[3] for k in keys) and any(r[6] < r[2] and r[6] for r in t['records'])
        spans = [t['records'][r + 1][0] - t['records'][r][0] for r in range(n - 1)]
        assert max(spans) > 40                                            # many lines


# ---------------------------------------------------------------------------
# membership
# ---------------------------------------------------------------------------

def _lists(t):
    names = [k[0] for k in t['keys']]
    words = [t['records'][k[1]][7] for k in t['keys']]
    half = names[::2]
    return {
        'empty': [],
        'everything': names + words,
        'half_duplicated': half + half + words[1::4] * 3,
        'absent': [n + b'?' for n in names] + [b'absent', b'A' * 2000],
        'empty_name': [b''],
        'prefix_pairs': [n[:-1] for n in names if n] + [n + b'x' for n in names[:50]] +
                        [w[:1] for w in words[:50]],
    }


@pytest.mark.parametrize('n,shape', [(257, 'mix'), (4099, 'distinct'), (65, 'one'), (1, 'mix')],
                         ids=lambda v: str(v))
def test_membership_equals_the_restatement(n, shape):
    text, t = world(n, shape)
    recs = _native(text)
    try:
        for label, names in _lists(t).items():
            for first_word in (False, True):
                got = recs.exclude(names, first_word=first_word)
                assert got.dtype == bool
                assert got.tolist() == fe.member(t, names, first_word), (label, first_word)
        if shape == 'mix' and n > 1:
            assert not all(fe.member(t, [b''], True))  # a key without a word is the empty word
    finally:
        recs.close()


def _keys_in_buckets_of_their_own(bits, count):
    keys, taken = [], set()
    for k in range(100000):
        name = 'key_%d of %d' % (k, k % 7)
        bucket = py2order.str_hash(name) & ((1 << bits) - 1)
        if bucket not in taken:
            taken.add(bucket)
            keys.append(b(name))
        if len(keys) == count:
            return keys
    raise AssertionError('not enough keys')


def test_list_names_that_share_buckets_change_nothing():
    keys = _keys_in_buckets_of_their_own(8, 100)
    text = b''.join(b'>' + k + b'\nACGT\n' for k in keys)
    t = fe.table(text, PARAMS, hash_bits=8)
    assert t['verdict'] is None
    words = [k.split()[0] for k in keys]
    listed = keys[::3] + [b'other_%d' % i for i in range(3000)] + words[1::5] * 4
    buckets = {fe.str_hash(n) & 255 for n in listed}
    assert len(buckets) == 256 and len(listed) > 8 * 256  # every run of equal hashes is long
    narrow, wide = _native(text, hash_bits=8), _native(text)
    try:
        _assert_equals_table(narrow, t)
        for first_word in (False, True):
            want = fe.member(t, listed, first_word)
            assert 0 < sum(want) < len(want)
            assert narrow.exclude(listed, first_word=first_word).tolist() == want
            assert wide.exclude(listed, first_word=first_word).tolist() == want
    finally:
        narrow.close()
        wide.close()


def test_two_keys_in_one_bucket_decline_the_text():
    text, t = world(257, 'distinct')
    narrow = fe.table(text, PARAMS, hash_bits=8)
    assert narrow['verdict'][0] == 'hash_collision' and narrow['verdict'][1] > 1
    assert engine.FastaRecords.parse(text, hash_bits=8) == (None, 'hash_collision')
    assert engine.FastaRecords.declined_line == narrow['verdict'][1]
    one, _ = world(257, 'one')  # a single key collides with nothing
    recs = _native(one, hash_bits=1)
    recs.close()
    assert recs.n_keys == 1


# ---------------------------------------------------------------------------
# the reflow
# ---------------------------------------------------------------------------

@pytest.mark.parametrize('n,shape', [(257, 'mix'), (4099, 'distinct'), (256, 'one'), (1, 'one')],
                         ids=lambda v: str(v))
def test_render_is_byte_equal_in_both_styles_and_orders(n, shape):
    text, t = world(n, shape)
    names = [k[0] for k in t['keys']]
    recs = _native(text)
    try:
        assert recs.render(np.arange(n), 'tab').tobytes() == fe.expected_tab(text)[0]
        assert recs.render([], 'tab').tobytes() == b'\n' == fe.expected_tab(b'')[0]
        assert recs.render([], 'fasta').tobytes() == b''
        first = fe.lines_of(text)[0]
        assert recs.render([0], 'tab').tobytes().startswith(first[1:-1] + b'\t')
        keys = recs.keys()
        for listed in ([], names[1:], names):  # all, one and no record kept
            keep = recs.exclude(listed)
            for order in fe.ORDERS:
                last, kept = keys['last_record'], keep
                if order == 'py2':
                    perm = engine.py2_order_of_hashes(keys['hash'])
                    last, kept = last[perm], keep[perm]
                got = recs.render(last[kept], 'fasta').tobytes()
                assert (got, None) == fe.expected_exclude(text, listed, False, order)
                assert int(kept.sum()) == len(names) - len(listed)
    finally:
        recs.close()


def test_one_record_in_the_tab_style_is_a_text_of_its_own():
    text = b'>only one\r\nAC\r\nGT'
    recs = _native(text)
    try:
        assert recs.render([0], 'tab').tobytes() == b'only one\tACGT\n' == fe.expected_tab(text)[0]
        assert recs.render([0, 0], 'fasta').tobytes() == b'>only one\nACGT\n' * 2
    finally:
        recs.close()


# ---------------------------------------------------------------------------
# declines, limits, arguments
# ---------------------------------------------------------------------------

def _declined(text, **kw):
    got = engine.FastaRecords.parse(text, **kw)
    assert isinstance(got, tuple) and got[0] is None, got
    return got[1], engine.FastaRecords.declined_line


def test_every_reason_comes_with_its_line():
    text, t = world(65, 'mix')
    B, cap = PARAMS['text_block'], PARAMS['max_name']
    lines = [ln for _, ln in t['lines']]
    assert _declined(b'ACGT\n' + text) == ('leading_text', 1)
    assert _declined(b'\n' + text) == ('leading_text', 1)
    # a CR in mid-line: in the first name, in a sequence line, in the last line with two
    # bytes; and as a block's last byte before a base
    two = [k for k, ln in enumerate(lines) if len(fe._payload(ln)) >= 2]
    for k in (two[0], two[len(two) // 2], two[-1]):
        bad = lines[:k] + [lines[k][:1] + b'\r' + lines[k][1:]] + lines[k + 1:]
        assert _declined(b''.join(bad)) == ('stray_cr', k + 1) == fe.table(b''.join(bad))['verdict']
    assert two[0] == 0 and len(lines[0]) + len(lines[1]) == B
    bad = b''.join([lines[0], lines[1][:-1] + b'\rA\n'] + lines[2:])
    assert bad[B - 1:B + 1] == b'\rA' and _declined(bad) == ('stray_cr', 2)
    two_crs = text + b'\r\r'
    assert _declined(two_crs) == ('stray_cr', len(lines)) == fe.table(two_crs)['verdict']
    ok = _native(text + b'\r')  # the text's last byte may be a CR
    ok.close()
    # the longest name goes native, one byte more does not
    at = t['records'][40][0]
    for extra, verdict in ((0, None), (1, ('long_name', at + 1))):
        long_name = b'>' + b'n' * (cap + extra) + b'\r\n'
        trial = b''.join(lines[:at] + [long_name] + lines[at + 1:])
        assert fe.table(trial, PARAMS)['verdict'] == verdict
        if verdict is None:
            recs = _native(trial)
            try:
                _assert_equals_table(recs, fe.table(trial, PARAMS))
            finally:
                recs.close()
        else:
            assert _declined(trial) == verdict
    # on one line the CR comes first
    both = b''.join(lines[:at] + [b'>' + b'n' * (cap + 1) + b'\rx\n'] + lines[at + 1:])
    assert _declined(both) == ('stray_cr', at + 1)
    assert _declined(text, max_bytes=len(text) - 1) == ('too_large', 0)
    assert _declined(text, max_bytes=1) == ('too_large', 0)
    ok = _native(text, max_bytes=len(text))
    ok.close()


def test_a_text_no_device_holds_is_declined_before_it_is_read():
    L, ctx = engine._lib.lib(), engine._lib.default_context()
    h, reason, line = ctypes.c_void_p(), ctypes.c_uint32(), ctypes.c_uint64()
    buf = np.frombuffer(b'>a\nAC\n', np.uint8)
    for max_bytes in (0, 1 << 40):
        rc = L.magot_fastarec_parse(ctx.handle, buf.ctypes.data, 1 << 50, 64, max_bytes,
                                    ctypes.byref(h), ctypes.byref(reason), ctypes.byref(line))
        assert rc == engine._lib.ERR_UNSUPPORTED and not h.value
        assert engine._lib.FASTAREC_REASONS[reason.value] == 'too_large' and line.value == 0


def test_two_to_the_31_lines_are_too_many():
    """Line numbers are 32-bit: the limit shows only at this size.  The text
    is an empty header and 2^31 - 1 empty lines, 2 GiB and a byte; it is
    declined after the count, before anything is sized by its lines."""
    text = np.full((1 << 31) + 1, 10, np.uint8)
    text[0] = ord('>')
    assert _declined(text) == ('too_many_lines', 0)


def test_arguments_are_checked_before_any_launch():
    L, ctx = engine._lib.lib(), engine._lib.default_context()
    h, reason, line = ctypes.c_void_p(), ctypes.c_uint32(), ctypes.c_uint64()
    rc = L.magot_fastarec_parse(ctx.handle, None, 10, 64, 0, ctypes.byref(h), ctypes.byref(reason),
                                ctypes.byref(line))
    assert rc == engine._lib.ERR_ARG and not h.value
    for bits in (0, 65, 1 << 20):
        with pytest.raises(engine.MagotError, match='hash_bits'):
            engine.FastaRecords.parse(b'>a\nAC\n', hash_bits=bits)
    recs = _native(b'>a\nAC\n>b\nGG\n')
    try:
        for bad in ([2], [0, 1, 2], [0xffffffff]):
            with pytest.raises(engine.MagotError, match='beyond'):
                recs.render(bad, 'tab')
        with pytest.raises(KeyError):
            recs.render([0], 'gff')
        blob, keep = np.frombuffer(b'ab', np.uint8), np.zeros(2, np.uint8)
        for off in ([0, 3], [1, 0], [0, 2, 1]):
            off = np.array(off, np.uint64)
            rc = L.magot_fastarec_exclude(ctx.handle, recs.handle, blob.ctypes.data, 2,
                                          off.ctypes.data, len(off) - 1, 0, keep.ctypes.data)
            assert rc == engine._lib.ERR_RANGE
        assert recs.exclude([b'a']).tolist() == [False, True]
    finally:
        recs.close()


def test_time_names_every_pass_and_the_answers_stand():
    text, t = world(4099, 'mix')
    recs = _native(text)
    try:
        got = recs.time(1)
        assert set(got) == set(engine.FastaRecords.PASSES) | {'text_bytes', 'reflow_bytes'}
        assert got['text_bytes'] == len(text)
        assert got['reflow_bytes'] == len(fe.expected_tab(text)[0])
        assert all(got[k] > 0 for k in engine.FastaRecords.PASSES)
        _assert_equals_table(recs, t)
        assert recs.render(np.arange(4099), 'tab').tobytes() == fe.expected_tab(text)[0]
    finally:
        recs.close()
    empty = _native(b'')
    try:
        assert all(v == 0 for v in empty.time(1).values())
        assert (empty.n_lines, empty.n_records, empty.n_keys) == (0, 0, 0)
        assert empty.exclude([b'a']).tolist() == [] and empty.render([], 'tab').tobytes() == b'\n'
    finally:
        empty.close()


# ---------------------------------------------------------------------------
# the recorded runs and the command line
# ---------------------------------------------------------------------------

def _call(fn, capfdbinary, *args, **kw):
    exc = None
    try:
        fn(*args, **kw)
    except Exception as e:  # noqa: BLE001
        exc = type(e).__name__
    return capfdbinary.readouterr().out.decode('latin-1'), exc


def _write_case(tmp_path, case):
    path = str(tmp_path / 'records.fa')
    with open(path, 'wb') as fh:
        fh.write(b(case['fasta']))
    if case['kind'] == 'literal':
        return path, case['list']
    list_path = str(tmp_path / 'names.txt')
    with open(list_path, 'wb') as fh:
        fh.write(b(case['list']))
    return path, list_path


@pytest.mark.parametrize('name', NAMES)
def test_goldens_on_both_paths_in_both_orders(name, tmp_path, capfdbinary):
    case = GOLD[name]
    path, arg = _write_case(tmp_path, case)
    flag = 'True' if case['first_word'] else 'False'
    why = None if case['path'] == 'native' else case['path']
    for order in fe.ORDERS:
        want = (case['out_py2'] if order == 'py2' else case['out'], case['exc'])
        tool = genome_tools.exclude_from_fasta
        assert _call(tool, capfdbinary, path, arg, flag, order=order) == want
        assert tool.last_path == ('exclude_from_fasta', 'native' if why is None else 'host', why)
        assert _call(tool, capfdbinary, path, arg, flag, order=order, native='False') == want
        assert tool.last_path == ('exclude_from_fasta', 'host', "native != 'True'")
    why = None if case['tab_path'] == 'native' else case['tab_path']
    want = (case['tab_out'], case['tab_exc'])
    assert _call(genome_tools.fasta2tab, capfdbinary, path) == want
    assert genome_tools.fasta2tab.last_path == \
        ('fasta2tab', 'native' if why is None else 'host', why)
    assert _call(genome_tools.fasta2tab, capfdbinary, path, native='False') == want
    if case['path'] not in ('native', 'a key without a word'):
        assert engine.FastaRecords.parse(b(case['fasta'])) == (None, case['path'])


def test_the_command_line_in_a_process_of_its_own(tmp_path):
    case = GOLD['random_4']
    assert case['path'] == 'native' and case['out_py2']
    path, arg = _write_case(tmp_path, case)
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get('PYTHONPATH', ''))
    argv = [sys.executable, '-m', 'magot_amd.genome_tools', 'exclude_from_fasta', path, arg]
    if case['first_word']:
        argv.append('just_firstword=True')
    res = subprocess.run(argv, stdout=subprocess.PIPE, stderr=subprocess.PIPE, env=env, timeout=300)
    assert res.returncode == 0, res.stderr[-2000:]
    assert res.stdout == b(case['out_py2'])
