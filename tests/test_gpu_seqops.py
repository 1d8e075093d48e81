"""revcomp_kernel, translate_kernel and codon_symbols_kernel (seqops.hip) against
the oracle beyond one block: the cases of tests/seqops_expect.py (a second
block and more, one record over several blocks, many records inside a chunk,
long runs of equal offsets, totals at and next to chunk and block multiples,
every byte value, mixed frames and strands, a caller's lut64, a full 32 KiB
symbol LUT), and the product paths (Sequence, any-library translate, cds2pep)
at the smallest sizes that leave one block.  Needs an MI355X: ``pytest -m gpu``.
"""

import contextlib
import io
import json
import os

import numpy as np
import pytest

import goldlib
import seqops_expect as se
from magot_amd import _lib, engine
from oracle import magot_oracle as mo

pytestmark = pytest.mark.gpu

GUARD = 64      # bytes of 0xEE past the end of an output buffer


@pytest.fixture(scope='module', autouse=True)
def _device():
    if _lib.lib().magot_device_count() <= 0:
        pytest.fail('no HIP device visible for a gpu test')


def _first_difference(got, want):
    for i, (g, w) in enumerate(zip(got, want)):
        if g != w:
            if g is None or w is None:
                return 'record %d: %r instead of %r' % (i, g and g[:40], w and w[:40])
            k = next((k for k, (a, b) in enumerate(zip(g, w)) if a != b), min(len(g), len(w)))
            return 'record %d of %d (lengths %d, %d) at %d: %r instead of %r' % (
                i, len(want), len(g), len(w), k, g[k:k + 20], w[k:k + 20])
    return 'lengths %d, %d' % (len(got), len(want))


def _same(got, want):
    want = list(want)
    assert got == want, _first_difference(got, want)


def _guarded(total):
    return np.full(total + GUARD, 0xEE, dtype=np.uint8)


# ---------------------------------------------------------------------------
# revcomp_kernel
# ---------------------------------------------------------------------------

@pytest.mark.parametrize('name', sorted(se.RC_CASES))
def test_revcomp_batch_vs_oracle(name):
    for recs, want in se.rc_case(name):
        _same(engine.revcomp_batch(list(recs)), want)


def _revcomp_abi(recs):
    """magot_revcomp_batch into a guarded buffer: (status, the whole buffer)."""
    buf, off = engine._concat(recs)
    out = _guarded(len(buf))
    rc = _lib.lib().magot_revcomp_batch(_lib.default_context().handle,
                                        _lib.ptr(buf) if len(buf) else None, _lib.ptr(off),
                                        len(recs), _lib.ptr(out))
    return rc, out, len(buf)


@pytest.mark.parametrize('name', ['rc_lengths', 'rc_totals'])
def test_revcomp_abi_writes_its_bytes_and_no_more(name):
    for recs, want in se.rc_case(name):
        rc, out, total = _revcomp_abi(recs)
        _lib.check(rc, 'magot_revcomp_batch')
        assert out[:total].tobytes().decode('latin-1') == ''.join(want), total
        assert (out[total:] == 0xEE).all(), total


def test_revcomp_abi_empty_batches_touch_nothing():
    for recs, _ in se.rc_case('rc_empty'):
        rc, out, total = _revcomp_abi(recs)
        assert rc == 0 and total == 0
        assert (out == 0xEE).all()


# ---------------------------------------------------------------------------
# translate_kernel
# ---------------------------------------------------------------------------

@pytest.mark.parametrize('name', sorted(se.TR_CASES))
def test_translate_batch_vs_oracle(name):
    for b, want in se.tr_case(name):
        got = engine.translate_batch(b['seqs'], b['frames'], b['strands'], lut64=b['lut64'])
        _same(got, want)


@pytest.mark.parametrize('name', ['tr_totals', 'tr_sparse'])
def test_translate_abi_writes_its_bytes_and_no_more(name):
    L = _lib.lib()
    for b, want in se.tr_case(name):
        n = len(b['seqs'])
        buf, off = engine._concat(b['seqs'])
        fr = np.asarray(b['frames'], dtype=np.int32)
        st = np.frombuffer(''.join(b['strands']).encode('ascii'), dtype=np.uint8).copy()
        poff = np.empty(n + 1, dtype=np.uint64)
        codons = np.empty(n, dtype=np.int64)
        _lib.check(L.magot_translate_sizes(_lib.ptr(off), n, _lib.ptr(fr), _lib.ptr(poff),
                                           _lib.ptr(codons)), 'magot_translate_sizes')
        assert poff.tolist() == se.pep_offsets(want)
        assert codons.tolist() == [-1 if w is None else len(w) for w in want]
        total = int(poff[n])
        out = _guarded(total)
        _lib.check(L.magot_translate_batch(_lib.default_context().handle, _lib.ptr(buf),
                                           _lib.ptr(off), n, _lib.ptr(fr), _lib.ptr(st), None,
                                           _lib.ptr(poff), _lib.ptr(out)), 'magot_translate_batch')
        assert out[:total].tobytes().decode('latin-1') == ''.join(w or '' for w in want), total
        assert (out[total:] == 0xEE).all(), total


# ---------------------------------------------------------------------------
# codon_symbols_kernel
# ---------------------------------------------------------------------------

@pytest.mark.parametrize('n_codons,K', se.SYM_CASES)
def test_codon_symbols_vs_definition(n_codons, K):
    seq, cls, K, lut = se.sym_case(n_codons, K)
    got = engine.codon_symbols(seq, cls, K, lut)
    want = se.symbols(seq, cls, K, lut)
    bad = [k for k in range(n_codons) if got[k] != want[k]]
    assert len(got) == n_codons and not bad, '%d of %d differ, first at codon %d' % (
        len(bad), n_codons, bad[0])


# ---------------------------------------------------------------------------
# the product paths at the same sizes
# ---------------------------------------------------------------------------

def test_sequence_over_two_blocks():
    from magot_amd.genome import Sequence
    s = se.product_seq()
    got = Sequence(s).reverse_compliment()
    assert isinstance(got, Sequence)
    _same([str(got)], [mo.reverse_complement(s)])
    for frame in range(5):
        for strand in '+-':
            for trim in (True, False):
                got = Sequence(s).translate(frame=frame, strand=strand, trimX=trim)
                want = mo.translate(s, frame=frame, strand=strand, trimX=trim)
                assert got == want, (frame, strand, trim, _first_difference([got], [want]))


def _libraries():
    with open(os.path.join(goldlib.HERE, 'translate_lib.json')) as fh:
        d = json.load(fh)
    libs = {}
    for name, (base, extra) in d['libs'].items():
        lib = dict(mo.STANDARD_CODE) if base == 'standard' else {}
        lib.update(extra)
        libs[name] = lib
    return libs


LIBRARIES = _libraries()


def _outcome(fn):
    try:
        return fn(), None
    except Exception as e:  # noqa: BLE001
        return None, type(e).__name__


@pytest.mark.parametrize('name', sorted(LIBRARIES))
def test_any_library_translate_over_seven_blocks(name):
    """Sequence.translate(library=...) on 5,000 bases: about 1,666 codons, so
    codon_symbols_kernel runs 7 blocks; frames -6..6, both strands, trimX on
    and off, the reference's exception types included."""
    from magot_amd.genome import Sequence
    lib = LIBRARIES[name]
    s = se.product_seq()[:se.LIB_BASES]
    for frame in range(-6, 7):
        for strand in '+-':
            for trim in (True, False):
                want = _outcome(lambda: mo.translate(s, library=lib, frame=frame, strand=strand,
                                                     trimX=trim))
                got = _outcome(lambda: Sequence(s).translate(library=lib, frame=frame,
                                                             strand=strand, trimX=trim))
                assert got == want, (name, frame, strand, trim,
                                     _first_difference([got[0]], [want[0]]), got[1], want[1])


def _stdout_of(fn, *a):
    b = io.BytesIO()
    out = io.TextIOWrapper(b, encoding='latin-1', write_through=True)
    exc = None
    with contextlib.redirect_stdout(out):
        try:
            fn(*a)
        except Exception as e:  # noqa: BLE001
            exc = type(e).__name__
    out.flush()
    return b.getvalue().decode('latin-1'), exc


@pytest.mark.parametrize('eol', ['\n', '\r\n'])
@pytest.mark.parametrize('final_eol', [True, False])
def test_cds2pep_one_batch_of_2000_records(tmp_path, eol, final_eol):
    """genome_tools.cds2pep on 2,000 wrapped records of 0-400 bases: the one
    translate_kernel batch of about 130 KB of residues the tool launches."""
    from magot_amd import genome_tools
    path = tmp_path / 'cds.fa'
    path.write_bytes(se.cds_fasta(eol, final_eol).encode('latin-1'))
    want = io.StringIO()
    mo.cds2pep(str(path), out=want)
    got, exc = _stdout_of(genome_tools.cds2pep, str(path))
    assert exc is None
    assert got.count('\n') == want.getvalue().count('\n')
    assert got == want.getvalue()
