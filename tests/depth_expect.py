"""What depth_from_gff must print (genome_tools.py:598-652), restated over
numpy prefix sums, a seeded generator of depth tables and GFFs, and the loader
of the reference's own recorded results (tests/golden/depth_from_gff.json,
written by golden/make_golden_depth.py).  Not a test module:
test_depth_host.py and test_gpu_depth.py import it, and so does the golden
generator, for the one table generator both sides use."""

import hashlib
import json
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, 'golden')
OBIROI_FA = 'O.biroi_refseqGenomeSubset.fasta'
OBIROI_GFF = 'O.biroi_NCBIrefseq_gff3Subset.gff'


def load():
    with open(os.path.join(GOLDEN, 'depth_from_gff.json')) as fh:
        return json.load(fh)


def sha(data):
    if isinstance(data, str):
        data = data.encode('latin-1')
    return hashlib.sha256(data).hexdigest()


# -- depth tables -----------------------------------------------------------

def formula_depths(n, mul, mod, add=0):
    """depth of position 1..n: (mul * pos + add) % mod"""
    return ((np.arange(1, n + 1, dtype=np.int64) * mul + add) % mod).astype(np.int64)


def table_text(contigs, sep=b'\t', eol=b'\n', final_eol=True):
    """The table of [(name, depths array)], one run per contig, positions from
    1; bytes."""
    parts = []
    for name, depths in contigs:
        nm = name.encode('latin-1') if isinstance(name, str) else name
        pos = np.arange(1, len(depths) + 1)
        parts.append(b''.join(nm + sep + b'%d' % p + sep + b'%d' % d + eol
                              for p, d in zip(pos.tolist(), np.asarray(depths).tolist())))
    text = b''.join(parts)
    if not final_eol and text.endswith(eol):
        text = text[:-len(eol)]
    return text


def spec_table(spec):
    """A table from a JSON-able spec {'contigs': [[name, n], ..], 'mul', 'mod'}:
    contig k's depths are formula_depths(n, mul, mod, add=3 * k).  (bytes,
    [(name, depths)])"""
    contigs = [(nm, formula_depths(n, spec['mul'], spec['mod'], 3 * k))
               for k, (nm, n) in enumerate(spec['contigs'])]
    return table_text(contigs), contigs


def fasta_lengths(path):
    """[(name, bases)] of a FASTA, names cut at the first blank."""
    out = []
    with open(path, 'rb') as fh:
        for line in fh:
            if line[:1] == b'>':
                out.append([line[1:].split()[0].decode('latin-1'), 0])
            else:
                out[-1][1] += len(line.strip())
    return out


def obiroi_spec():
    return {'contigs': fasta_lengths(os.path.join(GOLDEN, OBIROI_FA)), 'mul': 7, 'mod': 41}


# -- GFFs the restatement understands ----------------------------------------

def gff_text(transcripts, eol='\n'):
    """transcripts: [(id, seqid, strand, [(start, end), ..])] -> GFF3 with one
    mRNA line and its CDS lines each."""
    out = []
    for tid, seqid, strand, cds in transcripts:
        lo = min([c[0] for c in cds] or [1])
        hi = max([c[1] for c in cds] or [1])
        out.append('%s\tsrc\tmRNA\t%d\t%d\t.\t%s\t.\tID=%s' % (seqid, lo, hi, strand, tid))
        for k, (a, b) in enumerate(cds):
            out.append('%s\tsrc\tCDS\t%d\t%d\t.\t%s\t0\tID=%s.c%d;Parent=%s'
                       % (seqid, a, b, strand, tid, k, tid))
    return ''.join(ln + eol for ln in out)


def _slice_sum(prefix, a, b):
    """sum(arr[a:b]) from arr's prefix sums (len(arr) + 1 entries), a, b >= 0"""
    lo, hi = slice(a, b).indices(len(prefix) - 1)[:2]
    return int(prefix[max(hi, lo)] - prefix[lo])


def expected(contigs, transcripts, features, stream_length, cds_order, tx_order, parent_order,
             missing_order):
    """(text, exception name): what the reference prints for a table of
    [(name, depths)] (one run each, positions from 1) and ``transcripts`` as
    gff_text takes them, all coordinates >= 1 and strands '+' / '-'.
    ``cds_order`` lists (transcript index, cds index) in the CDS table's
    iteration order, ``tx_order`` transcript indices in the transcript
    table's; ``parent_order`` / ``missing_order`` map the first-occurrence
    lists to the per-parent dict's and the missing set's order."""
    prefix = {nm: np.concatenate([[0], np.cumsum(np.asarray(d, dtype=np.int64))])
              for nm, d in contigs}
    L = int(stream_length)
    out, missing, covsum = [], [], None
    try:
        if 'CDS' in features:
            out.append('#CDS counts\n')
            totals = {}
            for t, k in cds_order:
                tid, seqid, _, cds = transcripts[t]
                if seqid in prefix:
                    covsum = _slice_sum(prefix[seqid], cds[k][0] - 1, cds[k][1])
                else:
                    missing.append(tid + ' on ' + seqid)
                if covsum is None:
                    raise UnboundLocalError
                totals[tid] = totals.get(tid, 0) + covsum
            out += ['%s\t%d\n' % (p, totals[p]) for p in parent_order(list(totals))]
        if 'upstream' in features:
            out.append('#upstream ' + stream_length + 'bp counts\n')
            for t in tx_order:
                tid, seqid, strand, cds = transcripts[t]
                lo, hi = min(c[0] for c in cds), max(c[1] for c in cds)
                a, b = (max(0, lo - 1 - L), lo - 1) if strand == '+' else (hi, hi + L)
                if seqid in prefix:
                    covsum = _slice_sum(prefix[seqid], a, b)
                else:
                    missing.append(tid + ' on ' + seqid)
                if covsum is None:
                    raise UnboundLocalError
                out.append('%s\t%d\n' % (tid, covsum))
        if missing:
            out.append('#missing from depth file\n')
            out += [m + '\n' for m in missing_order(list(dict.fromkeys(missing)))]
    except UnboundLocalError:
        return ''.join(out), 'UnboundLocalError'
    return ''.join(out), None


def random_case(rng):
    """One small seeded case: (contigs [(name, depths)], transcripts, features,
    stream_length).  Some transcripts sit on contigs the table lacks, some
    CDS and flanks reach past their contig's end."""
    n_contigs = int(rng.integers(1, 4))
    contigs = [('c%d' % (k + 1), rng.integers(0, 50, int(rng.integers(1, 120))))
               for k in range(n_contigs)]
    seqids = [nm for nm, _ in contigs] + ['gone1', 'gone2']
    transcripts = []
    for t in range(int(rng.integers(1, 7))):
        seqid = seqids[int(rng.integers(0, len(seqids)))] if rng.random() < 0.8 else 'c1'
        cds = []
        for _ in range(int(rng.integers(1, 5))):
            a = int(rng.integers(1, 130))
            cds.append((a, a + int(rng.integers(0, 40))))
        transcripts.append(('t%d' % (t + 1), seqid, '+-'[int(rng.integers(0, 2))], cds))
    features = [['CDS', 'upstream'], ['CDS'], ['upstream'],
                ['CDS', 'intron', 'upstream', 'downstream']][int(rng.integers(0, 4))]
    return contigs, transcripts, features, str(int(rng.integers(0, 60)))


def case_inputs(case):
    """(depth table bytes, gff path or bytes) of a golden case"""
    if 'depth_spec' in case:
        depth = spec_table(case['depth_spec'])[0]
        assert sha(depth) == case['depth_sha']
    else:
        depth = case['depth'].encode('latin-1')
    if 'gff_file' in case:
        return depth, os.path.join(GOLDEN, case['gff_file'])
    return depth, case['gff'].encode('latin-1')


def case_files(case, tmp_path):
    """(depth path, gff path) of a golden case, written under tmp_path"""
    depth, gff = case_inputs(case)
    dp = os.path.join(str(tmp_path), 'depth.txt')
    with open(dp, 'wb') as fh:
        fh.write(depth)
    if isinstance(gff, bytes):
        gp = os.path.join(str(tmp_path), 'in.gff')
        with open(gp, 'wb') as fh:
            fh.write(gff)
        gff = gp
    return dp, gff


def same_as_recorded(out, exc, rec):
    """stdout bytes and exception name against one order's record"""
    assert exc == rec['exc']
    head, missing = split_missing(out.decode('latin-1'))
    assert sorted(missing) == rec['missing']
    if 'head' in rec:
        assert head == rec['head']
    else:
        assert (sha(head), len(head)) == (rec['sha'], rec['len'])


def split_missing(text):
    """(everything up to and with the '#missing from depth file' line, the
    set of lines after it): that block is a set's, its order no contract."""
    head, mark, tail = text.partition('#missing from depth file\n')
    return head + mark, frozenset(tail.splitlines())
