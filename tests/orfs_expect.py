"""What dna2orfs (reference genome_tools.py:145-180) writes, in closed form,
and the inputs the ORF-calling tests share (test infrastructure, CPU only).

The closed form, per contig, over ``oracle.magot_oracle.translate``:
  * streams in the reference's loop order j = 2*frame + (strand == '+');
  * a stream of n residues with s stops gives s + 1 ORFs (``split('*')``);
  * ORF i starts at residue k, one past the stop before it; its position is
    (frame on '+', len - frame on '-') + 3*k;
  * from_atg: 'M' + what follows the first M with every further M removed,
    'M' alone without one;
  * longest: the first ORF in loop order whose output string is longest;
  * a None stream raises AttributeError (after what was written before it),
    no longest candidate IndexError.
tests/test_orfs_expect.py pins it to tests/golden/dna2orfs.json, which
tests/golden/make_golden_orfs.py records from the reference itself.
"""

import hashlib
import random

from oracle import magot_oracle as mo

TILE = 1024  # engine.ORFCALL_TILE (asserted by the tests that import both)
LOOP = [(0, '-'), (0, '+'), (1, '-'), (1, '+'), (2, '-'), (2, '+')]
MODES = [(False, False), (True, False), (False, True), (True, True)]  # (from_atg, longest)


def sha(text):
    return hashlib.sha256(text.encode('latin-1')).hexdigest()


def output_string(orf, from_atg):
    if not from_atg:
        return orf
    i = orf.find('M')
    return 'M' if i < 0 else 'M' + orf[i + 1:].replace('M', '')


_SIX = {}


def six_frames(seq):
    """The six translate() results in loop order (computed once per sequence)."""
    if seq not in _SIX:
        _SIX[seq] = [mo.translate(seq, frame=f, strand=s) for f, s in LOOP]
    return _SIX[seq]


def contig_rows(seq, from_atg):
    """([(j, k, position, output string)] in loop order, first None stream or None)."""
    rows = []
    none_j = None
    six = six_frames(seq)
    for j, (frame, strand) in enumerate(LOOP):
        t = six[j]
        if t is None:
            if none_j is None:
                none_j = j
            continue
        assert none_j is None  # None streams are the last ones in loop order
        base = frame if strand == '+' else len(seq) - frame
        k = 0
        for orf in t.split('*'):
            rows.append((j, k, base + 3 * k, output_string(orf, from_atg)))
            k += len(orf) + 1
    return rows, none_j


def longest_row(rows):
    best = None
    for row in rows:
        if len(row[3]) > (len(best[3]) if best else 0):
            best = row
    return best


def block(name, seq, from_atg, longest):
    """(text dna2orfs writes for this contig, exception name or None)."""
    rows, none_j = contig_rows(seq, from_atg)
    exc = 'AttributeError' if none_j is not None else None
    if longest:
        if exc:
            return '', exc
        best = longest_row(rows)
        if best is None:
            return '', 'IndexError'
        return '>' + name + '_longestORF\n' + best[3] + '\n', None
    return ''.join('>%s-pos:%d\n%s\n' % (name, pos, out) for _, _, pos, out in rows), exc


def tool_text(contigs, from_atg, longest, order='insertion'):
    """(text, exception name or None) of dna2orfs over [(name, seq)]: blocks
    in dict order up to and including the first failing contig's."""
    seqs = {}
    for name, seq in contigs:  # GenomeSequence: a later record replaces an earlier one
        seqs[name] = seq
    names = mo.py2_dict_order(list(seqs)) if order == 'py2' else list(seqs)
    parts = []
    for name in names:
        text, exc = block(name, seqs[name], from_atg, longest)
        parts.append(text)
        if exc:
            return ''.join(parts), exc
    return ''.join(parts), None


def fasta(contigs, width=60):
    out = []
    for name, seq in contigs:
        out.append('>' + name + '\n')
        for i in range(0, len(seq), width):
            out.append(seq[i:i + width] + '\n')
    return ''.join(out)


def rc(seq):
    return mo.reverse_complement(seq)


def _rand(rnd, n, alphabet='ACGT'):
    return ''.join(rnd.choice(alphabet) for _ in range(n))


def _both(name, seq):
    return [(name, seq), (name + '_rc', rc(seq))]


def _codons(n, at):
    """n codons of GCC (A), with the codon at each index in ``at`` replaced."""
    c = ['GCC'] * n
    for i, v in at.items():
        c[i] = v
    return ''.join(c)


def case_all_lengths():
    rnd = random.Random(5200)
    return [('len%d' % n, _rand(rnd, n)) for n in range(5, 201)]


def case_short(n):
    rnd = random.Random(40 + n)
    return [('ok_a', _rand(rnd, 33)), ('ok_b', _rand(rnd, 7)), ('short%d' % n, _rand(rnd, n)),
            ('ok_c', _rand(rnd, 21))]


def case_chunk_edges():
    out = []
    at = {}
    for i in (15, 16, 17, TILE - 1, TILE, TILE + 1):
        at[i] = 'TAA'
        out += _both('stop%d' % i, _codons(TILE + 40, {i: 'TAA'}))
    out += _both('stops_all', _codons(TILE + 40, at))
    return out


def case_stream_edges():
    rnd = random.Random(77)
    body = _rand(rnd, 90)
    out = _both('stop_first', 'TAA' + body)
    out += _both('stop_last', body + 'TAA')
    out += _both('stop_both', 'TGA' + body + 'TAG')
    out += _both('stop_runs', _codons(40, {5: 'TAA', 6: 'TAG', 7: 'TGA', 8: 'TAA', 30: 'TAA',
                                          31: 'TAA'}))
    out += _both('taa_repeat', 'TAA' * 60)
    out += _both('taa_repeat_off', 'TAA' * 400 + 'T')
    out += _both('taa_dense', 'TAA' * (TILE + 70))  # more stops than one tile holds
    return out


def case_long_orf():
    # a stop-free stream of more than 2 tiles in all six frames, one stop near the far end
    return _both('long_open', _codons(2 * TILE + 320, {2 * TILE + 300: 'TAA'}))


def case_n_lower():
    rnd = random.Random(99)
    body = _rand(rnd, 120)
    out = [('n_start', 'N' + body), ('nnn_start', 'NNN' + body), ('n6_start', 'NNNNNN' + body),
           ('lower', body.lower()), ('mixed', _rand(rnd, 150, 'ACGTacgt')),
           ('n_inside', body[:40] + 'N' * 7 + body[40:]),
           ('n_end', body + 'NN'), ('n_sparse', _rand(rnd, 200, 'ACGTACGTACGTN')),
           ('iupac', _rand(rnd, 120, 'ACGTACGTRYKMn-'))]
    return out


def case_from_atg():
    out = []
    out += _both('m_none', _codons(30, {29: 'TAA'}))
    out += _both('m_one', _codons(30, {4: 'ATG', 29: 'TAA'}))
    out += _both('m_many', _codons(30, {0: 'ATG', 4: 'ATG', 5: 'ATG', 17: 'ATG', 28: 'ATG',
                                        29: 'TAA'}))
    out += _both('m_first_last', _codons(20, {0: 'ATG', 19: 'ATG'}))
    out += _both('m_per_orf', _codons(40, {3: 'ATG', 9: 'TAA', 19: 'TAG', 22: 'ATG', 23: 'ATG',
                                           30: 'TGA'}))
    # an M on each side of a tile boundary, and ORFs that carry it (or its
    # absence) across one and two boundaries
    out += _both('m_before_edge', _codons(TILE + 60, {TILE - 1: 'ATG', TILE + 50: 'TAA'}))
    out += _both('m_after_edge', _codons(TILE + 60, {TILE: 'ATG', TILE + 50: 'TAA'}))
    out += _both('m_both_edges', _codons(TILE + 60, {TILE - 1: 'ATG', TILE: 'ATG'}))
    out += _both('m_carried', _codons(2 * TILE + 90, {5: 'ATG', 2 * TILE + 40: 'TAA',
                                                      2 * TILE + 60: 'ATG'}))
    out += _both('m_not_carried', _codons(2 * TILE + 90, {5: 'ATG', 9: 'TAA',
                                                          2 * TILE + 40: 'ATG'}))
    out += _both('m_stop_then_edge', _codons(TILE + 60, {3: 'ATG', TILE - 2: 'TAA',
                                                         TILE + 5: 'ATG'}))
    return out


# longest ties.  ACROSS: the maximum (29) is attained in streams 0+ (j = 1) and
# 1- (j = 2) and not in 0-; in memory 1- lies before 0+, so loop order and
# memory order disagree.  ACROSS_ATG: the same with from_atg (40).  INSIDE /
# INSIDE_ATG: the maximum is attained twice inside one stream.  The tests
# assert these properties before they trust the cases.
TIE_ACROSS = ('AGTGACGCGCACTGCATCGATTGGTTCGATCGATCATTAGACCCTTATCTGACGCCGTCGAATGGAGTAGAGAATCCGCTTG'
              'CACCGTGA')
TIE_ACROSS_ATG = ('CACCGATGTCGACATATGCCGGTATTCCATAAGCCAGGTGATCAACAATTTTTCAGCAATCTCGACCCTAATTATGCT'
                  'TGTGAATGTTACTGTGCAAGCACCCAGCTCTTGAGAACGAGCTATCATGCAGTTGACTG')
TIE_INSIDE = ('AGGGGTCGACCTCAATTTTCGCTGAGATGCCCACGGGAATTAAGTAATTAATTCCGCACGACATACTCTAGGGGGCTCGCTTC'
              'ATCACTAATTTAACATCCCTATTGAGATGGCACGGTGATAGTCTCGCACCTGCAT')
TIE_INSIDE_ATG = ('CACCTGACTCAAGCGAGCACTAAGTCGTCTTTTGAGCGCATCAATCACTACGCACGCCGCTGATAGTCGACGAACGACA'
                  'TATCCTGTAGAGGTTCGCCGTGGTTGTCCAGTGAATAGTTT')


def longest_ties(seq, from_atg):
    """(maximum output length, the streams j of the rows that attain it)."""
    rows, _ = contig_rows(seq, from_atg)
    m = max(len(r[3]) for r in rows)
    return m, [r[0] for r in rows if len(r[3]) == m]


def case_ties():
    return [('tie_across', TIE_ACROSS), ('tie_across_atg', TIE_ACROSS_ATG),
            ('tie_inside', TIE_INSIDE), ('tie_inside_atg', TIE_INSIDE_ATG)]


def case_pos_width():
    rnd = random.Random(31)
    lens = [9, 10, 11, 99, 100, 101, 999, 1000, 1001, 9999, 10000, 10001]
    return [('w%d' % n, _rand(rnd, n)) for n in lens]


def case_six_digits():
    rnd = random.Random(32)
    return [('w120k', _rand(rnd, 120001))]


def case_names():
    rnd = random.Random(33)
    names = ['chr 1 some description', 'x' * 200, '', 'a\tb', 'scaffold_12|len=5', 'Z', 'zz top',
             'contig-pos:7', '>odd', 'ten']
    return [(nm, _rand(rnd, 40 + 3 * i)) for i, nm in enumerate(names)]


CASES = {
    'all_lengths': case_all_lengths,
    'short1': lambda: case_short(1), 'short2': lambda: case_short(2),
    'short3': lambda: case_short(3), 'short4': lambda: case_short(4),
    'chunk_edges': case_chunk_edges, 'stream_edges': case_stream_edges,
    'long_orf': case_long_orf, 'n_lower': case_n_lower, 'from_atg': case_from_atg,
    'ties': case_ties, 'pos_width': case_pos_width, 'six_digits': case_six_digits,
    'names': case_names,
}
