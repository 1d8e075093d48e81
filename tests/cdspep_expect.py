"""What the fused longest-ORF kernel (engine.LongestOrfs) must give for a
record, in closed form over ``oracle.magot_oracle``, and the inputs its tests
share (test infrastructure, CPU only).

The expected row of a record is the reference's own choice,
``Sequence.get_orfs(longest=True)`` (genome.py:824-851): the six translations
in loop order j = 2*frame + (strand == '+'), a None or empty one passed over,
each split at '*'; the first piece strictly longer than every piece before it.
``expected_row`` takes it from orfs_expect's rows (which also carry the stream
and the start residue) and checks it against ``mo.get_orfs``.  A record without
a non-empty piece has no row: the reference raises IndexError there.
"""

import random

import orfs_expect as oe
from oracle import magot_oracle as mo

BASES = 'ACGT'


def lut64_of(library):
    """The 64-byte table of a codon library: c0 + 4*c1 + 16*c2, A=0 C=1 G=2 T=3."""
    return bytes(bytearray(ord(library[BASES[i & 3] + BASES[(i >> 2) & 3] + BASES[i >> 4]])
                           for i in range(64)))


def expected_row(seq, library=None):
    """(j, k, orf) of the record's winner, or None when it has none."""
    if library is None:
        best = oe.longest_row(oe.contig_rows(seq, False)[0])
        best = (best[0], best[1], best[3]) if best else None
    else:
        best = None
        for j, (frame, strand) in enumerate(oe.LOOP):
            t = mo.translate(seq, library=library, frame=frame, strand=strand)
            if not t:
                continue
            k = 0
            for orf in t.split('*'):
                if len(orf) > (len(best[2]) if best else 0):
                    best = (j, k, orf)
                k += len(orf) + 1
        return best
    try:
        want = mo.get_orfs(seq, longest=True)
    except IndexError:
        want = None
    assert (best[2] if best else None) == want
    return best


def text_of(names, seqs, n_print):
    return ''.join('>' + nm + '\n' + (expected_row(s) or (0, 0, ''))[2] + '\n'
                   for nm, s in list(zip(names, seqs))[:n_print])


def codons(n, at, fill=('GCC',)):
    """n codons cycling through ``fill``, the codon at each index in ``at`` replaced."""
    c = [fill[i % len(fill)] for i in range(n)]
    for i, v in at.items():
        c[i] = v
    return ''.join(c)


def both(seq):
    return [seq, mo.reverse_complement(seq)]


def case_step_stops(S):
    """One stop at codon S-2, S-1, S, S+1, 2S-1 and 2S of frame 0, and all of
    them together, each on both strands."""
    at = (S - 2, S - 1, S, S + 1, 2 * S - 1, 2 * S)
    out = []
    for i in at:
        out += both(codons(2 * S + 9, {i: 'TAA'}))
    out += both(codons(2 * S + 9, dict((i, 'TAG') for i in at)))
    return out


def case_open_run(S):
    """GCC repeated is stop-free in all six frames (GCC CCG CGC / GGC GCG CGG):
    an open run across three steps, closed by one stop near the far end or by
    the stream's end."""
    return both(codons(3 * S + 20, {3 * S + 10: 'TAA'})) + both(codons(3 * S + 20, {}))


# Seven codons without a stop in frame 0 that put a stop into every other
# frame: TAA at offsets 1 and 2 ('+' frames 1 and 2), TTA at offsets 0, 1 and 2
# (TAA in each '-' frame).  Over this fill only frame 0 '+' has long runs.
QUIET = ('TTA', 'ATT', 'AAC', 'GCT', 'TAC', 'GTA', 'ACC')


def case_step_ties(S):
    """Two runs of the same, greatest length on either side of a step boundary
    of stream 1 (frame 0, '+'): a short run, a stop, m residues that end in step
    0, a stop at codon S-1 (then S), m residues that start in step 1, a stop, a
    short tail.  The first of the two wins; in the reverse complement the pair
    lies in stream 0, which meets them in the other order."""
    m = S - 3
    out = []
    for shift in (0, 1):
        a = S - 1 + shift - m - 1
        at = {a: 'TAA', a + m + 1: 'TGA', a + 2 * m + 2: 'TAG'}
        out += both(codons(a + 2 * m + 3 + 7, at, QUIET))
    return out


def tied_runs(seq):
    """(stream, [start residues]) of the rows of the record's greatest length."""
    rows = oe.contig_rows(seq, False)[0]
    m = max(len(r[3]) for r in rows)
    return m, [(r[0], r[1]) for r in rows if len(r[3]) == m]


def case_n_records():
    """'N' records without any candidate, and 'N'-led ones (the frame-0 trim)."""
    rnd = random.Random(611)
    body = ''.join(rnd.choice(BASES) for _ in range(90))
    return ['NNN', 'NNNN', 'NNNNN', 'N' + body, 'NN' + body, 'NNN' + body, 'NNNN' + body,
            'nnn' + body, body + 'N', body + 'NNN', 'NNNTAA', 'TAA', 'TAATAA', 'NNNTAAGCC',
            'GCCNNNGCC']


# ---------------------------------------------------------------------------
# The tool: get_CDS_peptides (reference genome_tools.py:283-321, read_gff3 read
# as read_gff) in closed form over the oracle's annotation model
# ---------------------------------------------------------------------------

INVALID_NAMES = "invalid option for 'names_from' argument\n"


def walk(fasta, gff, gene_name_filters=(), gene_length_filter=None, names_from='CDS',
         order='py2'):
    """([(name, CDS sequence, transcript number)] of the printed entries in
    output order up to the first exception, its name or None, stdout).  Where
    read_gff returns None, Genome.read_gff dies on ``None.genome = self``
    (genome.py:970-975) before the output file is opened: the entries are None."""
    import io
    printed = io.StringIO()
    aset = mo.read_gff(gff, out=printed)
    if aset is None:
        return None, 'AttributeError', printed.getvalue()
    aset.genome = mo.OracleGenome(mo.read_fasta(fasta))
    entries, tx_no = [], 0
    try:
        genes = list(aset.gene)
        if order == 'py2':
            genes = mo.py2_order_after_deepcopy(genes)
        for gene in genes:
            gene_obj = aset.gene[gene]
            keep = True
            for name_filter in gene_name_filters:
                if name_filter in gene_obj.ID:
                    keep = False
            if gene_length_filter is not None:
                fa = mo.get_fasta(gene_obj, aset, out=printed)
                if len(fa.split('\n')[1]) < int(gene_length_filter):
                    keep = False
            if not keep:
                continue
            for transcript in gene_obj.child_list:
                t_obj = aset.transcript[transcript]
                cds = {}
                for c in t_obj.child_list:
                    c_obj = aset.CDS[c]
                    seq = mo.get_seq(c_obj, out=printed)
                    if seq is None:
                        raise AttributeError('get_orfs')
                    mo.get_orfs(seq, longest=True)  # IndexError before anything of the transcript
                    cds[c_obj.coords] = (c_obj.ID, seq)
                keys = sorted(cds)
                if t_obj.strand == '-':
                    keys.reverse()
                for n, k in enumerate(keys):
                    if names_from == 'CDS':
                        name = cds[k][0]
                    elif names_from == 'transcript':
                        name = t_obj.ID + '-CDS' + str(n + 1)
                    elif names_from == 'gene':
                        name = gene_obj.ID + '-CDS' + str(n + 1)
                    else:
                        printed.write(INVALID_NAMES)
                        break
                    entries.append((name, cds[k][1], tx_no))
                tx_no += 1
    except Exception as e:  # noqa: BLE001
        return entries, type(e).__name__, printed.getvalue()
    return entries, None, printed.getvalue()


def tool_text(fasta, gff, **kw):
    """(what the tool writes, None when it opens no file; exception name or None)."""
    entries, exc, _ = walk(fasta, gff, **kw)
    if entries is None:
        return None, exc
    return ''.join('>' + nm + '\n' + mo.get_orfs(s, longest=True) + '\n'
                   for nm, s, _ in entries), exc


def _rand_dna(seed, n):
    import numpy as np
    idx = np.random.RandomState(seed).randint(0, 4, n)
    return np.frombuffer(b'ACGT', dtype=np.uint8)[idx].tobytes().decode('ascii')


def _line(seqid, ftype, lo, hi, strand, attrs):
    return '\t'.join([seqid, 'src', ftype, str(lo), str(hi), '.', strand, '.', attrs]) + '\n'


def synthetic_genome():
    a = _rand_dna(901, 3000)
    a = a[:1500] + 'NNN' + a[1503:]  # a CDS of NNN at 1501..1503
    return oe.fasta([('ctgA', a), ('ctgB', _rand_dna(902, 2400))])


def synthetic_gff(nnn=False, bad=None):
    """gene / transcript / CDS lines on both strands: duplicate coords, a '-'
    transcript with a '+' CDS, coords beyond the contig's end.  ``nnn`` puts a
    CDS over the planted NNN into the third gene's second transcript; ``bad``
    plants one diagnostic condition."""
    g = _line('ctgA', 'gene', 101, 900, '+', 'ID=geneA1')
    g += _line('ctgA', 'transcript', 101, 900, '+', 'ID=tA1.1;Parent=geneA1')
    g += _line('ctgA', 'CDS', 101, 250, '+', 'ID=cA1.1a;Parent=tA1.1')
    g += _line('ctgA', 'CDS', 400, 571, '+', 'ID=cA1.1b;Parent=tA1.1')
    g += _line('ctgA', 'CDS', 101, 250, '+', 'ID=cA1.1dup;Parent=tA1.1')  # replaces cA1.1a
    g += _line('ctgA', 'transcript', 101, 900, '+', 'ID=tA1.2;Parent=geneA1')
    g += _line('ctgA', 'CDS', 700, 900, '.', 'ID=cA1.2a;Parent=tA1.2')
    g += _line('ctgB', 'gene', 50, 2500, '-', 'ID=geneB')
    g += _line('ctgB', 'transcript', 50, 2500, '-', 'ID=tB.1;Parent=geneB')
    g += _line('ctgB', 'CDS', 50, 207, '-', 'ID=cB.1a;Parent=tB.1')
    g += _line('ctgB', 'CDS', 300, 480, '+', 'ID=cB.1plus;Parent=tB.1')  # '+' CDS, '-' transcript
    g += _line('ctgB', 'CDS', 2300, 2500, '-', 'ID=cB.1far;Parent=tB.1')  # ends beyond the contig
    g += _line('ctgA', 'gene', 1200, 2000, '+', 'ID=xgene3')
    g += _line('ctgA', 'transcript', 1200, 2000, '+', 'ID=t3.1;Parent=xgene3')
    g += _line('ctgA', 'CDS', 1200, 1290, '+', 'ID=c3.1a;Parent=t3.1')
    g += _line('ctgA', 'transcript', 1200, 2000, '+', 'ID=t3.2;Parent=xgene3')
    g += _line('ctgA', 'CDS', 1300, 1400, '+', 'ID=c3.2a;Parent=t3.2')
    if nnn:
        g += _line('ctgA', 'CDS', 1501, 1503, '+', 'ID=c3.2nnn;Parent=t3.2')
    g += _line('ctgA', 'CDS', 1600, 1711, '+', 'ID=c3.2b;Parent=t3.2')
    g += _line('ctgA', 'gene', 2100, 2900, '-', 'ID=gene4')
    g += _line('ctgA', 'transcript', 2100, 2900, '-', 'ID=t4.1;Parent=gene4')
    g += _line('ctgA', 'CDS', 2100, 2300, '-', 'ID=c4.1a;Parent=t4.1')
    g += _line('ctgA', 'CDS', 2500, 2630, '-', 'ID=c4.1b;Parent=t4.1')
    if bad == 'gene_child':      # a gene child that is no transcript: KeyError
        g += _line('ctgA', 'mRNA', 2100, 2900, '-', 'ID=m4;Parent=gene4')
    elif bad == 'transcript_child':  # a transcript child that is no CDS: KeyError
        g += _line('ctgA', 'UTR', 2650, 2700, '-', 'ID=u4;Parent=t4.1')
    elif bad == 'seqid':
        g += _line('ctgZ', 'CDS', 2700, 2800, '-', 'ID=c4.z;Parent=t4.1')
    elif bad == 'strand':
        g += _line('ctgA', 'CDS', 2700, 2800, '?', 'ID=c4.q;Parent=t4.1')
    elif bad == 'no_second_line':  # a gene without children: get_fasta() is ''
        g += _line('ctgB', 'gene', 1, 40, '+', 'ID=gene5')
    elif bad == 'no_annotations':
        # a parent without a line of its own: read_gff prints and returns None, so
        # the annotations have no gene, transcript or CDS dict (AttributeError)
        g += _line('ctgB', 'CDS', 600, 700, '+', 'ID=c9;Parent=ghost')
    return g


def no_cds_gff():
    """gene and transcript lines without any CDS line: AnnotationSet.__init__
    (genome.py:529-534) made the CDS dict all the same, no transcript has a
    child, and the tool writes an empty file without raising."""
    return ''.join(line + '\n' for line in synthetic_gff().split('\n') if '\tCDS\t' not in line
                   and line)


DIAGNOSTICS = {'gene_child': 'KeyError', 'transcript_child': 'KeyError', 'seqid': 'AttributeError',
               'strand': 'AttributeError', 'no_second_line': 'IndexError',
               'no_annotations': 'AttributeError'}

# name -> (gff builder or fixture file name, fasta builder or fixture file name, keywords)
TOOL_CASES = {
    'basic': (synthetic_gff, synthetic_genome, {}),
    'names_transcript': (synthetic_gff, synthetic_genome, {'names_from': 'transcript'}),
    'names_gene': (synthetic_gff, synthetic_genome, {'names_from': 'gene'}),
    'names_invalid': (synthetic_gff, synthetic_genome, {'names_from': 'exon'}),
    'filter_string': (synthetic_gff, synthetic_genome, {'gene_name_filters': 'xB'}),
    'filter_list': (synthetic_gff, synthetic_genome, {'gene_name_filters': ['gene4', 'eA']}),
    'length_below': (synthetic_gff, synthetic_genome, {'gene_length_filter': '322'}),
    'length_above': (synthetic_gff, synthetic_genome, {'gene_length_filter': '323'}),
    'nnn_middle': (lambda: synthetic_gff(nnn=True), synthetic_genome, {}),
    'no_annotations': (lambda: synthetic_gff(bad='no_annotations'), synthetic_genome, {}),
    'no_cds_lines': (no_cds_gff, synthetic_genome, {}),
    'c14': ('StandardGTF.gtf', lambda: oe.fasta([('Chromosome14', _rand_dna(14, 8589052))]), {}),
    'obiroi': ('O.biroi_NCBIrefseq_gff3Subset.gff', 'O.biroi_refseqGenomeSubset.fasta', {}),
}


def tool_inputs(name, golden_dir):
    """(fasta text, gff text, keywords) of a case."""
    import os
    gff, fa, kw = TOOL_CASES[name]
    texts = []
    for src in (fa, gff):
        if callable(src):
            texts.append(src())
        else:
            with open(os.path.join(golden_dir, src), encoding='latin-1', newline='') as fh:
                texts.append(fh.read())
    return texts[0], texts[1], dict(kw)


def case_lengths():
    """(contig, [(start, length, rc)]) with every length 0..200 on both strands
    at starts that walk through every byte phase."""
    rnd = random.Random(612)
    contig = ''.join(rnd.choice(BASES) for _ in range(48000))
    recs = []
    pos = 0
    for n in range(0, 201):
        for rc in (False, True):
            pos += (len(recs) * 7 - pos) % 16  # record i starts at phase 7i mod 16
            recs.append((pos, n, rc))
            pos += n
    assert pos < len(contig)
    return contig, recs
