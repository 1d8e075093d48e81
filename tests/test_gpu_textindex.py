"""The byte index of the resident-text tools (csrc/textindex.hip), on its own.

magot_debug_text_index uploads `len` bytes and indexes the first `index_len` of
them in plain mode.  The expectation is numpy's: the offsets where the byte
occurs in buf[:index_len].  The lengths sit around the 16-byte lane, the
1024-byte wave and the 4096-byte block; every one is run with nothing behind the
text and with 40 bytes of the indexed byte behind it, which must not be counted.
Line mode and the stray-CR check are pinned by the tests of the four tools.
"""
import ctypes

import numpy as np
import pytest

from magot_amd import _lib

pytestmark = pytest.mark.gpu

BLOCK = 4096
LENGTHS = (0, 1, 15, 16, 17, 31, 32, 33, 1023, 1024, 1025, 4095, 4096, 4097, 8191, 8192, 8193,
           3 * BLOCK + 5)
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
