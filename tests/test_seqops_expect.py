"""The shared inputs of the raw-string batch kernel tests (tests/seqops_expect.py)
hold the property each case is named for, so that a later edit cannot make a
case easier unnoticed; and the numpy symbol definition agrees with the oracle.
CPU only."""

import numpy as np
import pytest

import seqops_expect as se
from oracle import magot_oracle as mo


def _lens(batch):
    return [len(s) for s in batch]


def test_geometry_constants():
    assert (se.CHUNK, se.WAVE, se.BLOCK, se.SYM_BLOCK) == (16, 1024, 4096, 256)
    assert se.SYM_LUT_CAP == 32 ** 3


def test_any_byte_pool():
    s = se.any_bytes(np.random.default_rng(1), 200000)
    b = np.frombuffer(s.encode('latin-1'), np.uint8)
    assert len(b) == 200000 and len(set(b.tolist())) == 256
    common = np.isin(b, np.frombuffer(se.COMMON.encode('ascii'), np.uint8)).mean()
    assert 0.45 < common < 0.60     # half, plus the pool's own 11 / 256


def test_expected_values_are_the_oracle_s():
    for name in se.RC_CASES:
        for recs, want in se.rc_case(name):
            assert len(recs) == len(want)
    (recs, want), = se.rc_case('rc_all_bytes')
    assert want[0] == mo.reverse_complement(recs[0])
    # bytes >= 0x80 reverse-complement to 'n' and translate to 'X'
    assert mo.reverse_complement('\x80\xff') == 'nn'
    assert mo.translate('A\x80GAC\xff', trimX=False) == 'XX'


def test_rc_all_bytes():
    (recs, _), = se.rc_case('rc_all_bytes')
    assert len(recs) == 1
    b = recs[0].encode('latin-1')
    assert len(b) == 512 and all(b.count(bytes([v])) == 2 for v in range(256))


def test_rc_lengths():
    batches = se.rc_case('rc_lengths')
    assert [_lens(recs) for recs, _ in batches] == [[n] for n in se.RC_LENGTHS]
    for n in (0, 1, 15, 16, 17, 31, 32, 33, se.WAVE - 1, se.WAVE, se.WAVE + 1, se.BLOCK - 1,
              se.BLOCK, se.BLOCK + 1, 3 * se.BLOCK + 5):
        assert n in se.RC_LENGTHS
    last = se.RC_LENGTHS[-1]
    assert -(-last // se.BLOCK) == 4 and last % se.CHUNK     # four blocks, a tail chunk


def test_rc_many_tiny():
    (recs, _), = se.rc_case('rc_many_tiny')
    lens = _lens(recs)
    assert len(lens) == 3000 and min(lens) == 0 and max(lens) == 5
    assert lens[:3] == [0, 0, 0] and lens[-3:] == [0, 0, 0]
    off = se.offsets(lens)
    assert off[-1] > se.BLOCK
    assert se.longest_equal_run(off) >= 21          # 20 empty records in a row
    assert se.max_boundaries_in_a_chunk(off) >= 4
    # a run of empty records lies in each block the batch covers
    empty_at = {off[i] // se.BLOCK for i in range(3, len(lens) - 3) if lens[i] == 0}
    assert empty_at >= {0, 1}


def test_rc_totals():
    batches = se.rc_case('rc_totals')
    assert [sum(_lens(recs)) for recs, _ in batches] == \
        [se.BLOCK, se.BLOCK + 1, se.BLOCK + 16, 2 * se.BLOCK - 1, 16]
    assert all(len(recs) > 1 for recs, _ in batches)
    # what the last lane stores: nothing past a vector, one byte, a whole
    # vector, 15 bytes, one vector alone
    assert [t % se.CHUNK for t in se.RC_TOTALS] == [0, 1, 0, 15, 0]


def test_rc_empty():
    (a, wa), (b, wb) = se.rc_case('rc_empty')
    assert a == () and wa == ()
    assert len(b) > 1 and set(b) == {''} and set(wb) == {''}


def _tr(name):
    return se.tr_case(name)


def test_tr_grid():
    (b, want), = _tr('tr_grid')
    triples = set(zip(map(len, b['seqs']), b['frames'], b['strands']))
    assert triples == {(n, f, st) for n in range(41) for f in range(8) for st in '+-'}
    assert len(b['seqs']) == 41 * 8 * 2
    for s, f, w in zip(b['seqs'], b['frames'], want):
        assert (w is None) == (len(s) <= 2 + f)
    # shuffled: frames and strands alternate inside chunks
    assert b['frames'][:16] != sorted(b['frames'][:16])
    poff = se.pep_offsets(want)
    assert se.max_boundaries_in_a_chunk(poff) >= 4
    mixed = 0       # neighbours of another frame or strand that begin in one chunk
    for i in range(len(want) - 1):
        if want[i] and want[i + 1] and poff[i] // se.CHUNK == poff[i + 1] // se.CHUNK and \
                (b['frames'][i], b['strands'][i]) != (b['frames'][i + 1], b['strands'][i + 1]):
            mixed += 1
    assert mixed >= 10


def test_tr_long():
    (b, want), = _tr('tr_long')
    triples = set(zip(map(len, b['seqs']), b['frames'], b['strands']))
    assert triples == {(3 * se.BLOCK * 2 + d, f, st) for d in (0, 1, 2, 7) for f in (0, 1, 2)
                       for st in '+-'}
    # two blocks of residues a record, one fewer or a few more, placed so that every record
    # but the first, which starts a block, lies over three blocks
    lens = [len(w) for w in want]
    assert min(lens) == 2 * se.BLOCK - 1 and max(lens) > 2 * se.BLOCK
    poff = se.pep_offsets(want)
    assert all((poff[i + 1] - 1) // se.BLOCK - poff[i] // se.BLOCK >= 2
               for i in range(1, len(want)))


def test_tr_sparse():
    (b, want), = _tr('tr_sparse')
    assert len(want) == 4000 and max(map(len, b['seqs'])) == 5 and set(b['frames']) == {0, 1, 2}
    assert set(b['strands']) == {'+', '-'}
    assert all(w is None for w in want[:10]) and all(w is None for w in want[-10:])
    assert sum(1 for w in want if not w or len(w) <= 1) > len(want) * 0.8
    poff = se.pep_offsets(want)
    assert poff[-1] > se.WAVE
    assert se.longest_equal_run(poff) >= 21
    assert se.max_boundaries_in_a_chunk(poff) >= 4


def test_tr_all_bytes():
    (b, want), = _tr('tr_all_bytes')
    assert _lens(b['seqs']) == [300] * 64
    assert set(zip(b['frames'], b['strands'])) == {(f, st) for f in (0, 1, 2) for st in '+-'}
    seen = set(''.join(b['seqs']).encode('latin-1'))
    assert len(seen) == 256
    joined = ''.join(want)
    assert 'X' in joined and len(set(joined) - {'X'}) >= 20     # real residues too


def test_tr_lut():
    (b, want), = _tr('tr_lut')
    codons = se.lut_codons()
    assert sorted(codons) == sorted(mo.STANDARD_CODE) and len(set(codons)) == 64
    assert codons[1] == 'CAA' and codons[4] == 'ACA' and codons[16] == 'AAC'    # c0 is the fastest
    assert b['lut64'] == bytes(range(0x40, 0x80))
    assert b['library'] == {c: chr(0x40 + i) for i, c in enumerate(codons)}
    assert set(b['strands']) == {'+', '-'} and set(b['frames']) == {0}
    index_order = ''.join(chr(0x40 + i) for i in range(64))
    assert b['seqs'][0] == ''.join(codons) and want[0] == index_order
    assert b['seqs'][2] == mo.reverse_complement(b['seqs'][0])
    assert b['seqs'][4::2] == [b['seqs'][0].lower(), b['seqs'][2].lower()]
    assert b['seqs'][0::2] == b['seqs'][1::2] and b['strands'] == list('+-' * 4)
    # the '-' strand of the reverse complement reads the codons back in order
    minus_of_rc = [w for s, st, w in zip(b['seqs'], b['strands'], want)
                   if st == '-' and s.upper() == mo.reverse_complement(b['seqs'][0])]
    assert minus_of_rc == [index_order, index_order]
    assert all(len(w) == 64 for w in want)


def test_tr_totals():
    batches = _tr('tr_totals')
    assert [se.pep_offsets(want)[-1] for _, want in batches] == \
        [se.BLOCK, se.BLOCK + 1, 2 * se.BLOCK - 1]
    for b, want in batches:
        assert set(zip(b['frames'], b['strands'])) == {(f, st) for f in (0, 1, 2) for st in '+-'}
        assert any(w is None for w in want)
        assert se.longest_equal_run(se.pep_offsets(want)) >= 21


def test_none_first_and_last():
    (_, want), = _tr('tr_sparse')
    assert want[0] is None and want[-1] is None


def test_residue_count_helper_is_the_oracle_s():
    for n in range(0, 30):
        for f in range(0, 8):
            w = mo.translate('A' * n, frame=f, trimX=False)
            assert se.residues(n, f) == (None if w is None else len(w))


def test_symbol_cases():
    assert sorted(set(n for n, _ in se.SYM_CASES)) == [1, 255, 256, 257, 1000, 5000]
    assert sorted(set(K for _, K in se.SYM_CASES)) == [1, 5, 32]
    assert len(se.SYM_CASES) == 18
    for n, K in se.SYM_CASES:
        seq, cls, k, lut = se.sym_case(n, K)
        assert len(seq) == 3 * n and k == K and len(lut) == K ** 3 and len(cls) == 256
        assert int(cls.max()) < K
        if K > 1:
            assert len(set(cls.tolist())) == K
    assert 32 ** 3 == se.SYM_LUT_CAP
    seq, cls, K, lut = se.sym_case(5000, 32)
    assert len(set(seq)) == 256
    idx = se.symbol_index(seq, cls, K)
    assert idx.max() >= se.SYM_LUT_CAP - 256 and idx.min() < 256    # both ends of the full LUT
    # the index order matters to these inputs: another order gives other symbols
    c = np.asarray(cls)[np.frombuffer(seq, np.uint8)].astype(np.int64).reshape(-1, 3)
    other = np.asarray(lut)[c[:, 2] + K * c[:, 1] + K * K * c[:, 0]].tolist()
    assert other != se.symbols(seq, cls, K, lut)


def test_numpy_symbol_definition_equals_oracle_translate():
    rng = np.random.default_rng(9)
    seq = se.rand_over(rng, 3 * 500, 'ACGT')
    cls = np.full(256, 4, np.uint8)
    for i, ch in enumerate('ACGT'):
        cls[ord(ch)] = i
    K = 5
    lut = np.full(K ** 3, ord('X'), np.uint8)
    for codon, aa in mo.STANDARD_CODE.items():
        c0, c1, c2 = ('ACGT'.index(ch) for ch in codon)
        lut[c0 + K * c1 + K * K * c2] = ord(aa)
    got = ''.join(map(chr, se.symbols(seq.encode('ascii'), cls, K, lut)))
    assert got == mo.translate(seq, trimX=False)
    # and with the equivalent library of another table
    lib = {c: chr(0x40 + i) for i, c in enumerate(se.lut_codons())}
    for codon, v in lib.items():
        c0, c1, c2 = ('ACGT'.index(ch) for ch in codon)
        lut[c0 + K * c1 + K * K * c2] = ord(v)
    got = ''.join(map(chr, se.symbols(seq.encode('ascii'), cls, K, lut)))
    assert got == mo.translate(seq, library=lib, trimX=False)


def test_product_inputs():
    s = se.product_seq()
    assert len(s) == 3 * se.BLOCK * 2 + 7 and set(s) == set('ACGTacgtNnRY-')
    assert len(mo.translate(s, frame=0)) > 2 * se.BLOCK
    assert all(len(mo.translate(s, frame=f)) >= 2 * se.BLOCK for f in range(5))
    assert (se.LIB_BASES - 6) // 3 > 6 * se.SYM_BLOCK        # a seventh block of codons


@pytest.mark.parametrize('eol', ['\n', '\r\n'])
@pytest.mark.parametrize('final_eol', [True, False])
def test_cds_fasta(eol, final_eol):
    text = se.cds_fasta(eol, final_eol)
    assert text.count('>') == 2000 and text.startswith('ACGTTT' + eol + '>rec0 ')
    assert text.endswith(eol) == final_eol
    assert ('\r' in text) == (eol == '\r\n')
    bodies = text.split('>')[1:]
    lens = [len(''.join(b.split(eol)[1:])) for b in bodies]
    assert min(lens) == 0 and 0 < sorted(set(lens))[1] < 3 and max(lens) > 390
    assert 100000 < sum(n // 3 for n in lens) < 160000      # one batch of about 130 KB
