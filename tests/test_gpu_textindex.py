"""The byte index of the resident-text tools (csrc/textindex.hip), on its own.

magot_debug_text_index uploads `len` bytes and indexes the first `index_len` of
them in plain mode.  The expectation is numpy's: the offsets where the byte
occurs in buf[:index_len].  The lengths sit around the 16-byte lane, the
1024-byte wave and the 4096-byte block; every one is run with nothing behind the
text and with 40 bytes of the indexed byte behind it, which must not be counted.
The two line modes run through magot_debug_text_lines against the model of
tests/wavecopy_expect.py: the line starts of the same texts, and the stray-CR
check over one CR at every place where a lane, a wave or a block ends, and over
several.
"""
import ctypes

import numpy as np
import pytest

import wavecopy_expect as wx
from magot_amd import _lib

pytestmark = pytest.mark.gpu

BLOCK = wx.TEXT_BLOCK
LENGTHS = wx.TEXT_LENGTHS
PATTERNS = ('none', 'all', 'lane_last', 'lane_first', 'block_last', 'block_first', 'random')
FILL = ord('x')


def other_byte(byte):
    return ord('\t') if byte == ord('\n') else ord('\n')


def make_text(pattern, n, byte):
    """n bytes, and the second byte counted beside `byte` (-1: none)."""
    buf = np.full(n, FILL, dtype=np.uint8)
    at = np.arange(n)
    second = -1
    if pattern == 'all':
        buf[:] = byte
    elif pattern == 'lane_last':
        buf[at % 16 == 15] = byte
    elif pattern == 'lane_first':
        buf[at % 16 == 0] = byte
    elif pattern == 'block_last':
        buf[at % BLOCK == BLOCK - 1] = byte
    elif pattern == 'block_first':
        buf[at % BLOCK == 0] = byte
    elif pattern == 'random':
        # about 1/7 and 1/50: the four waves of a block hold different counts
        second = other_byte(byte)
        draw = np.random.RandomState(n * 7 + byte).randint(0, 350, size=n)
        buf[draw < 50] = byte
        buf[draw >= 343] = second
    return buf, second


def index(buf, index_len, byte, second):
    pos = np.full(max(index_len, 1), 2 ** 64 - 1, dtype=np.uint64)
    n, n2 = ctypes.c_uint64(), ctypes.c_uint64(2 ** 64 - 1)
    _lib.check(_lib.lib().magot_debug_text_index(
        _lib.default_context().handle, _lib.ptr(buf), len(buf), index_len, byte, second,
        _lib.ptr(pos), ctypes.byref(n), ctypes.byref(n2)), 'magot_debug_text_index')
    return pos, n.value, n2.value


@pytest.mark.parametrize('byte', (ord('\n'), ord('\t')), ids=('lf', 'tab'))
@pytest.mark.parametrize('pattern', PATTERNS)
def test_positions_and_counts_at_every_length(pattern, byte):
    for index_len in LENGTHS:
        text, second = make_text(pattern, index_len, byte)
        want = np.flatnonzero(text == byte).astype(np.uint64)
        want2 = int(np.count_nonzero(text == second)) if second >= 0 else 0
        for tail in (0, 40):
            # behind the text: the indexed byte, which a missing tail mask would count
            buf = np.concatenate([text, np.full(tail, byte, dtype=np.uint8)])
            pos, n, n2 = index(buf, index_len, byte, second)
            where = '%s, byte %d, index_len %d, len %d' % (pattern, byte, index_len, len(buf))
            assert n == len(want), where
            assert np.array_equal(pos[:n], want), where
            assert n2 == want2, where


def test_bad_arguments_are_refused():
    L = _lib.lib()
    ctx = _lib.default_context().handle
    buf = np.zeros(8, dtype=np.uint8)
    n = ctypes.c_uint64()
    for args in ((8, 9, 10, -1), (8, 8, 256, -1), (8, 8, 10, 256), (8, 8, 10, -2)):
        assert L.magot_debug_text_index(ctx, _lib.ptr(buf), *args, None, ctypes.byref(n),
                                        None) == _lib.ERR_ARG
    assert L.magot_debug_text_index(ctx, _lib.ptr(buf), 8, 8, 10, -1, None, None,
                                    None) == _lib.ERR_ARG


# --- the line modes -----------------------------------------------------------

UNTOUCHED = 2 ** 64 - 1


def lines(buf, index_len, check_cr, reason=0):
    """(pos with a sentinel behind what may be written, n_lines, the status word)"""
    pos = np.full(index_len + 3, UNTOUCHED, dtype=np.uint64)
    n, status = ctypes.c_uint64(UNTOUCHED), ctypes.c_uint64(0)
    _lib.check(_lib.lib().magot_debug_text_lines(
        _lib.default_context().handle, _lib.ptr(buf), len(buf), index_len, check_cr, reason,
        _lib.ptr(pos), ctypes.byref(n), ctypes.byref(status)), 'magot_debug_text_lines')
    return pos, n.value, status.value


def assert_lines(buf, index_len, check_cr, reason, where):
    want, n_lines, status = wx.lines_model(buf[:index_len], check_cr, reason)
    pos, n, got = lines(buf, index_len, check_cr, reason)
    where = '%s, check_cr %d, index_len %d, len %d' % (where, check_cr, index_len, len(buf))
    assert n == n_lines, where
    if n_lines:
        assert np.array_equal(pos[:n + 1], want), where
        assert pos[n] == index_len, where
    assert (pos[n + 1 if n else 0:] == UNTOUCHED).all(), where  # nothing else is written
    assert got == status, '%s: status %#x for %#x' % (where, got, status)
    return got


@pytest.mark.parametrize('check_cr', (0, 1))
@pytest.mark.parametrize('pattern', PATTERNS)
def test_line_starts_at_every_length(pattern, check_cr):
    for index_len in LENGTHS:
        text, second = make_text(pattern, index_len, wx.LF)
        if second >= 0:
            text[text == second] = wx.CR  # the random pattern: CRs at about 1/50
        for tail in (0, 40):
            # behind the text: LFs and CRs, which must not show
            assert_lines(np.concatenate([text, wx.TAIL[:tail]]), index_len, check_cr, 3, pattern)


def test_one_cr_at_every_place():
    """a CR is stray unless an LF follows it or it is the text's last byte,
    whatever lies behind the text; the byte behind a lane's last is another
    lane's, another wave's, another block's"""
    strays = 0
    for label, buf, index_len in wx.one_cr_cases():
        strays += assert_lines(buf, index_len, 1, 2, label) != wx.NO_STRAY
        assert lines(buf, index_len, 0, 2)[2] == wx.NO_STRAY, label
    assert strays > 50


def test_several_crs():
    """the lowest line wins over lanes, waves and blocks and inside a lane; of
    CR CR LF the first is stray; random texts over three blocks"""
    for label, text in wx.several_cr_cases():
        for reason in (2, 0xa5):
            got = assert_lines(text, len(text), 1, reason, label)
            assert got != wx.NO_STRAY and got & 0xff == reason, label
        assert_lines(text, len(text), 0, 2, label)


def test_line_mode_bad_arguments_are_refused():
    L = _lib.lib()
    ctx = _lib.default_context().handle
    buf = np.zeros(8, dtype=np.uint8)
    n = ctypes.c_uint64()
    assert L.magot_debug_text_lines(ctx, _lib.ptr(buf), 8, 9, 1, 0, None, ctypes.byref(n),
                                    None) == _lib.ERR_ARG
    assert L.magot_debug_text_lines(ctx, _lib.ptr(buf), 8, 8, 1, 256, None, ctypes.byref(n),
                                    None) == _lib.ERR_ARG
    assert L.magot_debug_text_lines(ctx, _lib.ptr(buf), 8, 8, 1, 0, None, None,
                                    None) == _lib.ERR_ARG
    assert L.magot_debug_text_lines(ctx, _lib.ptr(buf), 8, 8, 1, 0, None, ctypes.byref(n),
                                    None) == 0
    assert n.value == 1
