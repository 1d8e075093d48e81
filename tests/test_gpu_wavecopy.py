"""The grouped wave copies of csrc/wavecopy.h on their own, byte for byte
against the numpy models of tests/wavecopy_expect.py.

piece_group_copy runs through magot_debug_piece_copy (launch_piece_copy<16>, as
the FASTA reflow and the renamed text launch it), span_group_copy without text
parts through magot_copy_segments and with them through
magot_debug_text_assembly (launch_text_assembly, as magot_fasta_text_execute).
Every case is one launch.  The output buffer goes to the device prefilled and
comes back whole, and the whole of it is compared, its guard bytes included:
what no piece covers must come back as it went.  That the cases cover every
(source phase, destination phase, length) class, the second and third rounds
of the two loops and the X-trim at every alignment is asserted without a
device in test_wavecopy_expect.py."""

import ctypes
import functools

import numpy as np
import pytest
import torch

import wavecopy_expect as wx
from magot_amd import _lib, engine

pytestmark = pytest.mark.gpu


def same(got, want, where):
    bad = np.flatnonzero(got != want)
    assert not len(bad), '%s: %d of %d bytes differ, the first at %d (%d for %d)' % (
        where, len(bad), len(want), bad[0], got[bad[0]], want[bad[0]])


def piece_copy(case, base_len=None, out_len=None):
    """(status, the output buffer after the call)"""
    got = case.out.copy()
    rc = _lib.lib().magot_debug_piece_copy(
        _lib.default_context().handle, _lib.ptr(case.base),
        len(case.base) if base_len is None else base_len, _lib.ptr(case.src), _lib.ptr(case.dst),
        _lib.ptr(case.len), len(case.src), _lib.ptr(got), len(got) if out_len is None else out_len)
    return rc, got


def assert_piece_copy(case, where):
    rc, got = piece_copy(case)
    _lib.check(rc, 'magot_debug_piece_copy')
    same(got, case.model(), where)


def copy_segments(case):
    d_src = torch.from_numpy(case.src).cuda()
    d_dst = torch.from_numpy(case.dst).cuda()
    torch.cuda.synchronize()
    engine.copy_segments(d_src.data_ptr(), len(case.src), d_dst.data_ptr(), case.src_off,
                         case.dst_off)
    return d_dst.cpu().numpy()


def assert_segments(case, where):
    got = copy_segments(case)
    same(got, case.model(), where)
    first, last = int(case.dst_off[0]), int(case.dst_off[-1])
    assert np.array_equal(got[:first], case.dst[:first]), where  # before dst_off[0]
    assert np.array_equal(got[last:], case.dst[last:]) and len(got) - last == wx.GUARD, where


def assemble(case, protein, out_len=None, units=None, rspan=None, text_len=None, pay_len=None):
    """(status, the output buffer after the call, *written)"""
    got = case.out.copy()
    units = case.units if units is None else units
    rspan = case.rspan if rspan is None else rspan
    written = ctypes.c_uint64(2 ** 64 - 1)
    rc = _lib.lib().magot_debug_text_assembly(
        _lib.default_context().handle, _lib.ptr(units), len(units), _lib.ptr(case.text),
        len(case.text) if text_len is None else text_len, _lib.ptr(rspan), len(rspan) // 2,
        _lib.ptr(case.pay), len(case.pay) if pay_len is None else pay_len, protein, _lib.ptr(got),
        len(got) if out_len is None else out_len, ctypes.byref(written))
    return rc, got, written.value


def assert_assembly(case, protein, where):
    want, n = case.model(protein)
    rc, got, written = assemble(case, protein)
    _lib.check(rc, 'magot_debug_text_assembly')
    assert written == n, where
    same(got, want, where)
    return got


every_piece = functools.lru_cache(None)(wx.piece_every_class)
every_segment = functools.lru_cache(None)(wx.segment_every_class)
every_unit = functools.lru_cache(None)(wx.assembly_every_class)
xtrim = functools.lru_cache(None)(wx.assembly_xtrim)


# --- piece_group_copy ---------------------------------------------------------

def test_piece_copy_of_every_class():
    assert_piece_copy(every_piece(), 'every class')


def test_piece_copy_group_shapes():
    """one wave, one workgroup of four, the next workgroup; groups of empty
    pieces and empty pieces at a group's edges; no piece at all"""
    for name, case in sorted(wx.piece_shapes().items()):
        assert_piece_copy(case, name)
    rc, got = piece_copy(wx.piece_shapes()['n0'])
    assert rc == 0 and np.array_equal(got, wx.piece_shapes()['n0'].out)


def test_piece_copy_loop_rounds():
    """pieces of 4,200 and 8,400 bytes among tiny ones: the chunk loop's second
    and third round of 256 chunks"""
    assert_piece_copy(wx.piece_loops(), 'loop rounds')


def test_piece_copy_refuses_a_piece_outside_its_buffers():
    case = wx.piece_shapes()['n17']
    k = int(np.argmax(case.len))
    n = int(case.len[k])
    assert n > 1
    L = _lib.lib()
    for field, size in (('src', len(case.base)), ('dst', len(case.out))):
        for at in (size - n + 1, size + 1, 2 ** 63, 2 ** 64 - 1):
            bad = wx.PieceCase(case.base, case.src.copy(), case.dst.copy(), case.len, case.out)
            getattr(bad, field)[k] = at
            rc, got = piece_copy(bad)
            assert rc == _lib.ERR_RANGE, (field, at)
            assert 'piece %d' % k in L.magot_last_error().decode()
            assert np.array_equal(got, case.out), (field, at)
    # a buffer one byte short of its last piece
    rc, got = piece_copy(case, base_len=int((case.src + case.len).max()) - 1)
    assert rc == _lib.ERR_RANGE and np.array_equal(got, case.out)
    rc, got = piece_copy(case, out_len=int((case.dst + case.len).max()) - 1)
    assert rc == _lib.ERR_RANGE and np.array_equal(got, case.out)
    rc, got = piece_copy(case, out_len=1 << 28)
    assert rc == _lib.ERR_ARG and np.array_equal(got, case.out)
    _lib.check(piece_copy(case)[0], 'magot_debug_piece_copy')


# --- span_group_copy without text parts ---------------------------------------

def test_segments_of_every_class():
    assert_segments(every_segment(), 'every class')


def test_segments_group_shapes():
    for name, case in sorted(wx.segment_shapes().items()):
        assert_segments(case, name)


def test_segments_loop_rounds():
    assert_segments(wx.segment_loops(), 'loop rounds')


# --- span_group_copy with text parts ------------------------------------------

def test_assembly_of_every_class():
    case = every_unit()
    first = assert_assembly(case, 0, 'every class')
    again = assert_assembly(case, 0, 'every class, again')  # the same bytes on the same inputs
    assert np.array_equal(first, again)


def test_assembly_group_shapes():
    for name, case in sorted(wx.assembly_shapes().items()):
        assert_assembly(case, 0, name)
    none = wx.AssemblyCase(np.zeros(0, dtype=wx.UNIT_DTYPE), wx.noise(1, 16), [], wx.noise(2, 16),
                           wx.pattern(100))
    assert_assembly(none, 0, 'no unit')


def test_assembly_byte_loop_rounds():
    """16 units with 40 to 55 and with 70 to 85 bytes of text: more than 512 and
    more than 1,024 byte-stored bytes in one group"""
    assert_assembly(wx.assembly_byte_loops(), 0, 'byte loop rounds')


def test_assembly_chunk_loop_rounds():
    assert_assembly(wx.assembly_chunk_loops(), 0, 'chunk loop rounds')


@pytest.mark.parametrize('protein', (1, 0))
def test_assembly_x_trim(protein):
    """with protein a payload loses its leading X, which moves its source by a
    byte, at every alignment; without, the same tables keep it"""
    case = xtrim()
    got = assert_assembly(case, protein, 'X-trim, protein %d' % protein)
    assert np.array_equal(got, assert_assembly(case, protein, 'X-trim, again'))
    other, n_other = case.model(1 - protein)
    assert n_other != case.model(protein)[1] and not np.array_equal(got, other)


def test_assembly_refuses_what_lies_outside_its_buffers():
    case = xtrim()
    L = _lib.lib()
    refused = lambda **kw: assemble(case, 1, **kw)
    k = int(np.argmax(case.units['text_len']))
    units = case.units.copy()
    units['text_off'][k] = len(case.text) - int(units['text_len'][k]) + 1
    calls = [dict(units=units)]
    units = case.units.copy()
    units['text_off'][k] = 2 ** 64 - 1
    calls.append(dict(units=units))
    units = case.units.copy()
    units['rec'][np.flatnonzero(units['rec'] != wx.NO_RECORD)[0]] = len(case.rspan) // 2
    calls.append(dict(units=units))
    for span in ((len(case.pay) - 1, len(case.pay) + 1), (9, 8), (2 ** 63, 2 ** 63 + 1)):
        rspan = case.rspan.copy()
        rspan[4:6] = span
        calls.append(dict(rspan=rspan))
    calls.append(dict(pay_len=int(case.rspan.max()) - 1))
    calls.append(dict(text_len=int((case.units['text_off'] + case.units['text_len']).max()) - 1))
    n1, n0 = case.model(1)[1], case.model(0)[1]
    calls.append(dict(out_len=n1 - 1))  # the text is a byte longer than the buffer
    for kw in calls:
        rc, got, written = refused(**kw)
        assert rc == _lib.ERR_RANGE, sorted(kw)
        assert L.magot_last_error().decode().startswith('magot_debug_text_assembly')
        assert np.array_equal(got, case.out), sorted(kw)
    assert assemble(case, 0, out_len=n0 - 1)[0] == _lib.ERR_RANGE
    # the host's total follows the X-trim rule: what fits only with it is accepted
    assert n1 < n0
    rc, got, written = assemble(case, 1, out_len=n1)
    assert rc == 0 and written == n1
    same(got, case.model(1)[0], 'out_len is the text\'s length')
    assert assemble(case, 1, out_len=1 << 28)[0] == _lib.ERR_ARG
