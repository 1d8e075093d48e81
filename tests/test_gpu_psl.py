"""besthits_from_psl on the device (psl.hip; genome_tools.py:572-592):
engine.BestHits against the restated table of psl_expect.py on seeded worlds,
exactly; every run recorded from the reference through
genome_tools.besthits_from_psl on both paths and in both orders; the
verification of the grouping under a narrowed hash; the limits; one
command-line call.

Worlds: 0, 1, around a wave and around a workgroup of data lines, and 4099 (the
sort and the line index then span several blocks), each with one key for all
lines, all keys distinct, and a heavy-tailed mix with ties."""

import collections
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

import psl_expect as pe
from magot_amd import engine, genome_tools, py2order

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = pe.load()
NAMES = sorted(GOLD)
WORLDS = [(n, shape) for n in pe.SIZES for shape in pe.SHAPES]


def _native(text, **kw):
    """engine.BestHits of a text that must not be declined"""
    hits = engine.BestHits.parse(text, **kw)
    assert isinstance(hits, engine.BestHits), hits  # (None, reason): declined
    return hits


def _assert_equals_table(hits, text):
    want = pe.table(text)
    assert hits.n_lines == want['n_lines']
    assert hits.n_pass == len(want['pass']) and hits.n_groups == len(want['groups'])
    assert hits.n_data == want['n_lines'] - len(want['pass'])
    off, length = hits.pass_lines()
    assert off.dtype == length.dtype == np.uint64
    assert list(zip(off.tolist(), length.tolist())) == want['pass']
    g = hits.groups()
    for name, dtype in engine.BestHits.GROUP_COLUMNS:
        assert g[name].dtype == dtype and len(g[name]) == len(want['groups'])
    rows = list(zip(*[g[c].tolist() for c in ('first_line', 'best_line', 'score', 'off', 'len')]))
    assert rows == [r[1:] for r in want['groups']]
    assert g['hash'].tolist() == [py2order.str_hash(r[0].decode('latin-1'))
                                  for r in want['groups']]


@pytest.mark.parametrize('n_data,shape', WORLDS, ids=['%d-%s' % w for w in WORLDS])
def test_best_hits_equal_the_restated_table(n_data, shape):
    text = pe.world(n_data, shape)
    hits = _native(text)
    try:
        assert hits.n_data == n_data
        _assert_equals_table(hits, text)
    finally:
        hits.close()


def test_the_worlds_hold_what_they_promise():
    for n_data, shape in WORLDS:
        text = pe.world(n_data, shape)
        lines = pe.lines_of(text)
        starts = np.cumsum([0] + [len(ln) for ln in lines])
        assert (starts[1:-1] % pe.TEXT_BLOCK == 0).any()  # an LF ends a block, a line starts one
        assert max(len(ln) for ln in lines) > 8192
        assert sum(ln[:1] in pe.PASS_BYTES for ln in lines[1:-1]) >= 3  # header lines inside
        groups = pe.table(text)['groups']
        if shape == 'one':
            assert len(groups) == min(n_data, 1)
        if shape == 'distinct':
            assert len(groups) == n_data
        if shape != 'mix' or n_data < 255:
            continue
        data = [(k, ln.split(b'\t')) for k, ln in enumerate(lines) if ln[:1] not in pe.PASS_BYTES]
        score = {k: int(f[0]) - int(f[1]) for k, f in data}
        ties = 0
        lines_of_key = collections.defaultdict(list)
        for k, f in data:
            lines_of_key[f[9]].append(k)
        for key, first, best, top, _, _ in groups:
            at_top = [k for k in lines_of_key[key] if score[k] == top]
            assert best == at_top[0] and first <= best
            ties += len(at_top) > 1
        assert ties >= 3
        last_of = {f[9]: k for k, f in data}
        assert any(best == last_of[key] and first != best for key, first, best, *_ in groups)
        assert any(key.endswith(b'\n') for key, *_ in groups)  # a 10-field key
        assert min(score.values()) < 0 and 1 < len(groups) < n_data


# ---------------------------------------------------------------------------
# the recorded runs
# ---------------------------------------------------------------------------

def _tool(path, capfdbinary, **kw):
    exc = None
    try:
        genome_tools.besthits_from_psl(path, **kw)
    except Exception as e:  # noqa: BLE001
        exc = type(e).__name__
    return capfdbinary.readouterr().out.decode('latin-1'), exc


@pytest.mark.parametrize('name', NAMES)
def test_goldens_on_both_paths_in_both_orders(name, tmp_path, capfdbinary):
    case = GOLD[name]
    path = str(tmp_path / 'hits.psl')
    with open(path, 'wb') as fh:
        fh.write(case['text'].encode('latin-1'))
    why = None if case['path'] == 'native' else case['path']
    for order in ('py2', 'insertion'):
        want = case['out_py2'] if order == 'py2' and case['out_py2'] is not None else case['out']
        assert _tool(path, capfdbinary, order=order) == (want, case['exc'])
        assert genome_tools.besthits_from_psl.last_path == \
            ('besthits_from_psl', 'native' if why is None else 'host', why)
        assert _tool(path, capfdbinary, order=order, native='False') == (want, case['exc'])
        assert genome_tools.besthits_from_psl.last_path == \
            ('besthits_from_psl', 'host', "native != 'True'")
    if why is not None:
        assert engine.BestHits.parse(case['text'].encode('latin-1')) == (None, why)


# ---------------------------------------------------------------------------
# the verification of the grouping
# ---------------------------------------------------------------------------

def _lines_for(keys, rounds=3):
    return b''.join(pe.psl_line((7 * k + r) % 11, (3 * k) % 5, key)
                    for r in range(rounds) for k, key in enumerate(keys))


def test_two_keys_in_one_bucket_decline_the_text(tmp_path, capfdbinary):
    keys = ['query_%d' % k for k in range(200)]  # 200 keys in 64 buckets
    text = _lines_for(keys)
    assert engine.BestHits.parse(text, hash_bits=6) == (None, 'hash_collision')
    hits = _native(text)  # 64 bits: no two of them collide
    hits.close()
    assert hits.n_groups == 200
    # the tool's answer does not depend on which path gave it
    path = str(tmp_path / 'hits.psl')
    with open(path, 'wb') as fh:
        fh.write(text)
    for order in ('py2', 'insertion'):
        assert _tool(path, capfdbinary, order=order) == \
            (pe.expected(text, order).decode('latin-1'), None)


def test_keys_in_buckets_of_their_own_go_native_under_a_narrow_hash():
    keys, taken = [], set()
    for k in range(4000):
        bucket = py2order.str_hash('query_%d' % k) & 63
        if bucket not in taken:
            taken.add(bucket)
            keys.append('query_%d' % k)
    assert len(keys) == 64  # every bucket of the 6 bits holds one key
    text = _lines_for(keys, rounds=5)
    hits = _native(text, hash_bits=6)
    try:
        assert hits.n_groups == 64 and hits.n_data == 320
        _assert_equals_table(hits, text)
    finally:
        hits.close()


def test_a_single_key_goes_native_under_a_narrow_hash():
    text = pe.world(257, 'one')
    hits = _native(text, hash_bits=6)
    try:
        _assert_equals_table(hits, text)
        assert hits.n_groups == 1
    finally:
        hits.close()
    hits = _native(text, hash_bits=1)
    hits.close()


# ---------------------------------------------------------------------------
# limits, timing, arguments, the command line
# ---------------------------------------------------------------------------

def test_a_text_above_max_bytes_is_declined():
    text = pe.world(65, 'mix')
    assert engine.BestHits.parse(text, max_bytes=len(text) - 1) == (None, 'too_large')
    assert engine.BestHits.parse(text, max_bytes=1) == (None, 'too_large')
    hits = _native(text, max_bytes=len(text))
    hits.close()
    # Nothing of the text's size is allocated, and the text is not read, before
    # the decline: a length no device holds (2^50) is declined all the same,
    # where an allocation of it would fail with a HIP error.
    L, ctx = engine._lib.lib(), engine._lib.default_context()
    h, reason, line = ctypes.c_void_p(), ctypes.c_uint32(), ctypes.c_uint64()
    buf = np.frombuffer(text, np.uint8)
    for max_bytes in (0, 1 << 40):
        rc = L.magot_psl_parse(ctx.handle, buf.ctypes.data, 1 << 50, 64, max_bytes,
                               ctypes.byref(h), ctypes.byref(reason), ctypes.byref(line))
        assert rc == engine._lib.ERR_UNSUPPORTED and not h.value
        assert engine._lib.PSL_REASONS[reason.value] == 'too_large' and line.value == 0


def test_time_names_every_pass_and_the_answers_stand():
    text = pe.world(4099, 'mix')
    hits = _native(text)
    try:
        t = hits.time(1)
        assert set(t) == set(engine.BestHits.PASSES) | {'text_bytes'}
        assert t['text_bytes'] == len(text)
        assert all(t[k] > 0 for k in engine.BestHits.PASSES)
        _assert_equals_table(hits, text)
    finally:
        hits.close()
    empty = _native(b'')
    try:
        assert all(v == 0 for v in empty.time(1).values())
        assert (empty.n_lines, empty.n_groups) == (0, 0)
    finally:
        empty.close()


def test_arguments_are_checked_before_any_launch():
    L = engine._lib.lib()
    ctx = engine._lib.default_context()
    h, reason, line = ctypes.c_void_p(), ctypes.c_uint32(), ctypes.c_uint64()
    rc = L.magot_psl_parse(ctx.handle, None, 10, 64, 0, ctypes.byref(h), ctypes.byref(reason),
                           ctypes.byref(line))
    assert rc == engine._lib.ERR_ARG and not h.value
    for bits in (0, 65, 1 << 20):
        with pytest.raises(engine.MagotError, match='hash_bits'):
            engine.BestHits.parse(b'psl\n', hash_bits=bits)


def test_the_command_line_in_a_process_of_its_own(tmp_path):
    case = GOLD['random_0']
    path = str(tmp_path / 'hits.psl')
    with open(path, 'wb') as fh:
        fh.write(case['text'].encode('latin-1'))
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get('PYTHONPATH', ''))
    res = subprocess.run([sys.executable, '-m', 'magot_amd.genome_tools', 'besthits_from_psl', path],
                         stdout=subprocess.PIPE, stderr=subprocess.PIPE, env=env, timeout=300)
    assert res.returncode == 0, res.stderr[-2000:]
    assert res.stdout == case['out_py2'].encode('latin-1')
