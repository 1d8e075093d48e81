"""Inputs and expected values the raw-string batch kernel tests share (test
infrastructure, CPU only): revcomp_kernel, translate_kernel and
codon_symbols_kernel of magot_amd/csrc/seqops.hip beyond one block.

The kernels are output-stationary: a lane owns CHUNK output bytes, a wave
WAVE, a 256-thread block BLOCK; codon_symbols_kernel is one lane per codon,
SYM_BLOCK codons per block.  The cases below are named for the property they
hold (tests/test_seqops_expect.py asserts each), with fixed seeds.

Expected values come from ``oracle.magot_oracle`` alone (reverse_complement,
translate with trimX=False and its ``library=``), and for the symbol kernel
from the definition in include/magot.h in numpy, lut[c0 + K*c1 + K*K*c2];
nothing here calls the product.
"""

import functools

import numpy as np

from oracle import magot_oracle as mo

LANES = 256                # threads of a block, one chunk each
CHUNK = 16                 # output bytes of a lane (one 16-byte store)
WAVE = 64 * CHUNK          # 1024
BLOCK = LANES * CHUNK      # 4096
SYM_BLOCK = 256            # codons of a codon_symbols_kernel block
SYM_LUT_CAP = 32768        # the ABI's cap on K**3

COMMON = 'ACGTacgtNn-'
PRODUCT_ALPHABET = 'ACGTacgtNnRY-'


def any_bytes(rng, n):
    """n characters (latin-1, one per byte) over all 256 byte values, COMMON's
    drawn about half the time."""
    common = np.frombuffer(COMMON.encode('ascii'), np.uint8)
    pick = rng.random(n) < 0.5
    a = rng.integers(0, 256, n).astype(np.uint8)
    b = common[rng.integers(0, len(common), n)]
    return np.where(pick, b, a).astype(np.uint8).tobytes().decode('latin-1')


def rand_over(rng, n, alphabet):
    ab = np.frombuffer(alphabet.encode('latin-1'), np.uint8)
    return ab[rng.integers(0, len(ab), n)].tobytes().decode('latin-1')


def offsets(lengths):
    """The n + 1 offset table of records of these lengths."""
    off = [0]
    for n in lengths:
        off.append(off[-1] + n)
    return off


def max_boundaries_in_a_chunk(off):
    """The most distinct record boundaries strictly inside one chunk's span."""
    inner = sorted(set(o for o in off if o % CHUNK))
    best = run = 0
    last = None
    for o in inner:
        run = run + 1 if o // CHUNK == last else 1
        last = o // CHUNK
        best = max(best, run)
    return best


def longest_equal_run(off):
    best = run = 1
    for a, b in zip(off, off[1:]):
        run = run + 1 if a == b else 1
        best = max(best, run)
    return best


# ---------------------------------------------------------------------------
# reverse complement: name -> list of batches, a batch a list of strings
# ---------------------------------------------------------------------------

RC_LENGTHS = [0, 1, 15, 16, 17, 31, 32, 33, WAVE - 1, WAVE, WAVE + 1, BLOCK - 1, BLOCK, BLOCK + 1,
              3 * BLOCK + 5]
RC_TOTALS = [BLOCK, BLOCK + 1, BLOCK + 16, 2 * BLOCK - 1, 16]


def rc_all_bytes():
    return [[bytes(range(256)).decode('latin-1') * 2]]


def rc_lengths():
    rng = np.random.default_rng(6101)
    return [[any_bytes(rng, n)] for n in RC_LENGTHS]


def rc_many_tiny():
    rng = np.random.default_rng(6102)
    lens = rng.integers(0, 6, 3000)
    lens[:3] = 0
    lens[-3:] = 0
    for at in (40, 700, 1500, 2950):     # runs of empty records
        lens[at:at + int(rng.integers(20, 60))] = 0
    return [[any_bytes(rng, int(n)) for n in lens]]


def _records_to_total(rng, total, longest):
    """Record lengths 0..longest that sum to exactly ``total``."""
    lens = []
    left = total
    while left:
        n = min(int(rng.integers(0, longest + 1)), left)
        lens.append(n)
        left -= n
    return lens


def rc_totals():
    rng = np.random.default_rng(6103)
    out = []
    for total in RC_TOTALS:
        lens = _records_to_total(rng, total, 7 if total == 16 else 300)
        out.append([any_bytes(rng, n) for n in lens])
    return out


def rc_empty():
    return [[], [''] * 7]


RC_CASES = {'rc_all_bytes': rc_all_bytes, 'rc_lengths': rc_lengths, 'rc_many_tiny': rc_many_tiny,
            'rc_totals': rc_totals, 'rc_empty': rc_empty}


@functools.lru_cache(maxsize=None)
def rc_case(name):
    """((records, expected), ...) per batch of the case; computed once."""
    return tuple((tuple(b), tuple(mo.reverse_complement(s) for s in b)) for b in RC_CASES[name]())


# ---------------------------------------------------------------------------
# translate: name -> list of batches; a batch is a dict of seqs, frames,
# strands and, for a caller's table, lut64 with the oracle's library for it
# ---------------------------------------------------------------------------

TR_TOTALS = [BLOCK, BLOCK + 1, 2 * BLOCK - 1]
TR_LONG_BASE = 3 * BLOCK * 2
MOSTLY_ACGT = 'ACGT' * 5 + 'acgtNn'


def _batch(recs, lut64=None, library=None):
    return {'seqs': [r[0] for r in recs], 'frames': [r[1] for r in recs],
            'strands': [r[2] for r in recs], 'lut64': lut64, 'library': library}


def residues(length, frame):
    """Residues translate() emits before the trim, None where it returns None
    (oracle.magot_oracle.translate: one per position p in frame..length-1
    with (p + frame) % 3 == 2)."""
    if length <= 2 + frame:
        return None
    return sum(1 for p in range(frame, length) if (p + frame) % 3 == 2)


def tr_grid():
    rng = np.random.default_rng(6201)
    recs = [(rand_over(rng, n, MOSTLY_ACGT), f, st)
            for n in range(41) for f in range(8) for st in '+-']
    order = rng.permutation(len(recs))
    return [_batch([recs[i] for i in order])]


def tr_long():
    rng = np.random.default_rng(6202)
    recs = [(rand_over(rng, TR_LONG_BASE + d, MOSTLY_ACGT), f, st)
            for d in (7, 0, 1, 2) for f in (0, 1, 2) for st in '+-']
    return [_batch(recs)]


def tr_sparse():
    rng = np.random.default_rng(6203)
    lens = rng.integers(0, 6, 4000)
    lens[:10] = rng.integers(0, 3, 10)      # below one codon: None
    lens[-10:] = rng.integers(0, 3, 10)
    for at in (300, 1900, 3500):            # runs that give no residue
        lens[at:at + 40] = rng.integers(0, 3, 40)
    recs = [(rand_over(rng, int(n), MOSTLY_ACGT), int(rng.integers(0, 3)),
             '+-'[int(rng.integers(2))]) for n in lens]
    return [_batch(recs)]


def tr_all_bytes():
    rng = np.random.default_rng(6204)
    return [_batch([(any_bytes(rng, 300), i % 3, '+-'[(i // 3) % 2]) for i in range(64)])]


def lut_codons():
    """The 64 ACGT codons in the ABI's index order c0 + 4*c1 + 16*c2, A=0 C=1
    G=2 T=3 (include/magot.h)."""
    b = 'ACGT'
    return [b[i % 4] + b[(i // 4) % 4] + b[i // 16] for i in range(64)]


def tr_lut():
    codons = lut_codons()
    fwd = ''.join(codons)
    rev = mo.reverse_complement(fwd)
    recs = [(s, 0, st) for s in (fwd, rev, fwd.lower(), rev.lower()) for st in '+-']
    lut64 = bytes(0x40 + i for i in range(64))
    return [_batch(recs, lut64, {c: chr(0x40 + i) for i, c in enumerate(codons)})]


def tr_totals():
    rng = np.random.default_rng(6205)
    out = []
    for total in TR_TOTALS:
        recs = []
        left = total
        while left:
            n, f, st = int(rng.integers(0, 61)), int(rng.integers(0, 3)), '+-'[int(rng.integers(2))]
            if len(recs) % 50 == 10:        # a run of records that give None
                recs += [(rand_over(rng, int(rng.integers(0, 3)), 'ACGT'), f, st)] * 25
            c = residues(n, f) or 0
            if c > left:                    # close the batch: frame 0, 3 bases a residue
                n, f, c = 3 * left, 0, left
            recs.append((rand_over(rng, n, MOSTLY_ACGT), f, st))
            left -= c
        out.append(_batch(recs))
    return out


TR_CASES = {'tr_grid': tr_grid, 'tr_long': tr_long, 'tr_sparse': tr_sparse,
            'tr_all_bytes': tr_all_bytes, 'tr_lut': tr_lut, 'tr_totals': tr_totals}


@functools.lru_cache(maxsize=None)
def tr_case(name):
    """((batch, expected), ...) per batch of the case; expected holds the
    untrimmed translate() result of each record, None included."""
    out = []
    for b in TR_CASES[name]():
        want = tuple(mo.translate(s, library=b['library'], frame=f, strand=st, trimX=False)
                     for s, f, st in zip(b['seqs'], b['frames'], b['strands']))
        out.append((b, want))
    return tuple(out)


def pep_offsets(want):
    return offsets([len(w) if w else 0 for w in want])


# ---------------------------------------------------------------------------
# codon symbols: (n_codons, K) -> (seq, class256, K, lut), expected in numpy
# ---------------------------------------------------------------------------

SYM_CASES = [(n, K) for n in (1, SYM_BLOCK - 1, SYM_BLOCK, SYM_BLOCK + 1, 1000, 5000)
             for K in (1, 5, 32)]


@functools.lru_cache(maxsize=None)
def sym_case(n_codons, K):
    rng = np.random.default_rng(6300 + 100 * K + n_codons)
    seq = rng.integers(0, 256, 3 * n_codons).astype(np.uint8)
    cls = rng.integers(0, K, 256).astype(np.uint8)
    lut = rng.integers(0, 256, K ** 3).astype(np.uint8)
    for a in (seq, cls, lut):
        a.setflags(write=False)
    return seq.tobytes(), cls, K, lut


def symbol_index(seq, cls, K):
    c = np.asarray(cls)[np.frombuffer(seq, np.uint8)].astype(np.int64).reshape(-1, 3)
    return c[:, 0] + K * c[:, 1] + K * K * c[:, 2]


def symbols(seq, cls, K, lut):
    """out[k] = lut[c0 + K*c1 + K*K*c2], c = class256[byte] (include/magot.h)."""
    return np.asarray(lut)[symbol_index(seq, cls, K)].tolist()


# ---------------------------------------------------------------------------
# product paths at the same sizes
# ---------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def product_seq():
    """One sequence whose peptide covers more than two blocks."""
    return rand_over(np.random.default_rng(6401), TR_LONG_BASE + 7, PRODUCT_ALPHABET)


LIB_BASES = 5000    # about 1,666 codons: 7 blocks of codon_symbols_kernel


def cds_fasta(eol, final_eol, n_records=2000):
    """A CDS FASTA in 60-base lines: a sequence before the first header, empty
    records, records below one codon, records of up to 400 bases."""
    rng = np.random.default_rng(6402)
    lines = ['ACGTTT']
    for r in range(n_records):
        lines.append('>rec%d some description' % r)
        seq = rand_over(rng, int(rng.integers(0, 401)), 'ACGTacgtNRY*')
        for a in range(0, len(seq), 60):
            lines.append(seq[a:a + 60])
    return eol.join(lines) + (eol if final_eol else '')
