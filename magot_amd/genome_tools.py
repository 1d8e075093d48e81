"""Command-line tools on the extraction path (genome_tools.py of the reference).

    python -m magot_amd.genome_tools gff2fasta <fasta> <gff> [seq_type=protein]
           [longest=True] [genomic=True] [from_exons=True] [order=py2|insertion]
           [native=False]
    python -m magot_amd.genome_tools cds2pep <cds.fasta>
    python -m magot_amd.genome_tools extract_upstream_downstream <fasta> <gff> <length> up|down
           [feature_type=gene] [namefrom=ID] [truncate_names=True] [native=False]
    python -m magot_amd.genome_tools coords2fasta <fasta> <seqid> <start> <stop> [truncate_names=False]
    python -m magot_amd.genome_tools blast_csv2fasta <fasta> <blast.csv> [order=py2|insertion]
    python -m magot_amd.genome_tools exonerate2fasta <fasta> <exonerate.txt> [order=py2|insertion]
    python -m magot_amd.genome_tools get_seq_from_fasta <fasta> <seq_name> [truncate_names=False]
    python -m magot_amd.genome_tools dna2orfs <fasta> <out.fasta> [from_atg=1] [longest=1]
           [order=py2|insertion] [native=False]
    python -m magot_amd.genome_tools mask_from_gff <fasta> <gff> [mask_type=soft|hard]
           [overwrite_softmask=True] [feature_type=CDS] [order=py2|insertion] [native=False]
    python -m magot_amd.genome_tools at_content_from_fasta <fasta> [native=False]
    python -m magot_amd.genome_tools depth_from_gff <depth.txt> <gff> [features=['CDS','upstream']]
           [stream_length=1000] [order=py2|insertion] [native=False]
    python -m magot_amd.genome_tools fqstats <reads.fastq> [native=False]
    python -m magot_amd.genome_tools purge_overlaps <first.gff> <gff_to_purge> [native=False]
    python -m magot_amd.genome_tools besthits_from_psl <hits.psl> [order=py2|insertion]
           [native=False]
    python -m magot_amd.genome_tools composition_by_site <alignment.fasta> [order=py2|insertion]
           [native=False]
    python -m magot_amd.genome_tools heterozygosity_from_vcf <calls.vcf> [window=10000]
           [loci=<file, one locus per line>] [order=py2|insertion] [native=False]
    python -m magot_amd.genome_tools exclude_from_fasta <fasta> <names.txt | name,name,...>
           [just_firstword=True] [order=py2|insertion] [native=False]
    python -m magot_amd.genome_tools fasta2tab <fasta> [native=False]
    python -m magot_amd.genome_tools replace_names <text> <names.tsv> [name_end=';']
           [order=py2|insertion] [native=False]
    python -m magot_amd.genome_tools convert_gff <gff> gff3|gtf|augustus|RepeatMasker <gff3|gtf|exon_added_gff3>
           [order=py2|insertion] [native=False]
    python -m magot_amd.genome_tools tab2fasta <table.tab> [native=False]
    python -m magot_amd.genome_tools repeatmasker2augustushints <repeatmasker.gff> [native=False]
    python -m magot_amd.genome_tools get_CDS_peptides <fasta> <gff> <out.fasta>
           [gene_name_filters=<characters>] [gene_length_filter=<bases>]
           [names_from=CDS|transcript|gene] [order=py2|insertion] [native=False]

Arguments follow the reference's CLI convention (genome_tools.py:25-45):
positional values, then ``key=value`` pairs, all strings.  The reference
``eval``s the assembled call; here values are parsed as Python literals
(``True``/``False``/numbers) and never executed.  ``dna2orfs`` takes its two
switches by the reference's truthiness instead: any non-empty value, the text
``False`` included, switches them on (genome_tools.py:149, 165).

Record order defaults to ``py2`` so the bytes written match the reference's
own goldens (test_data/test_suite.py:12-13); ``order=insertion`` gives the
Python-3 order.
"""

import ast
import ctypes
import json
import os
import re
import sys
import time

import numpy as np

from . import engine
from . import genome
from .py2order import py2_float_str as _py2_float_str  # the rule genome.get_gff prints scores by


class _Clock(object):
    """Wall-clock phases of one CLI call, from the call's start: with
    MAGOT_CLI_TIMING=1 one JSON line on stderr (``{"cli_phases_s": ...}``);
    otherwise nothing is recorded.  ``at(name)`` stamps the time since the
    start (any thread); ``lap(name)`` the time since the previous lap."""

    def __init__(self):
        self.on = os.environ.get('MAGOT_CLI_TIMING') == '1'
        self.t0 = self.last = time.perf_counter()
        self.laps, self.stamps = {}, {}
        self.release_thread = None

    def lap(self, name):
        if self.on:
            t = time.perf_counter()
            self.laps[name] = self.laps.get(name, 0.0) + t - self.last
            self.last = t

    def at(self, name):
        if self.on:
            self.stamps[name] = time.perf_counter() - self.t0

    def emit(self):
        if self.on:
            sys.stderr.write(json.dumps({'cli_phases_s': self.laps, 'cli_stamps_s': self.stamps,
                                         'cli_total_s': time.perf_counter() - self.t0}) + '\n')
            sys.stderr.flush()


class _Release(object):
    """What one CLI call closes when it is done, in order.  ``later()``
    closes it on a background thread and returns that thread: once the
    text is in the caller's hands, freeing the device buffers and the
    planner's host tables (C3: ~0.12 s) need not delay it.  The thread is
    not a daemon, so an interpreter that exits first still waits for it."""

    def __init__(self):
        self.objs = []

    def add(self, obj):
        if obj is not None:
            self.objs.append(obj)
        return obj

    def now(self):
        objs, self.objs = self.objs, []
        for obj in objs:
            obj.close()

    def later(self):
        import threading
        th = threading.Thread(target=self.now, name='magot-release')
        th.start()
        return th


def _literal(text):
    try:
        return ast.literal_eval(text)
    except (ValueError, SyntaxError):
        return text


def _write(text):
    if getattr(sys.stdout, 'buffer', None) is not None:
        _write_bytes(text.encode('latin-1'))
    else:
        sys.stdout.write(text)


def _write_bytes(*parts):
    out = getattr(sys.stdout, 'buffer', None)
    if out is not None:
        sys.stdout.flush()
        for p in parts:
            # an unbuffered stream (PYTHONUNBUFFERED) writes what one write(2)
            # takes, at most 2 GiB, and says how much
            view = memoryview(p).cast('B')
            while len(view):
                n = out.write(view)
                view = view[len(view) if n is None else n:]
        out.flush()
    else:
        sys.stdout.write(''.join(bytes(p).decode('latin-1') for p in parts))


def gff2fasta(genome_sequence, gff, from_exons='False', seq_type='nucleotide', longest='False',
              genomic='False', order='py2', native='True'):
    """genome_tools.py:324-330.

    The native planner (magot_gff_plan: read_gff + get_fasta lowering in C++)
    and one kernel launch serve every combination of from_exons, genomic and
    longest; inputs that take one of the reference's diagnostic paths use the
    object path (``native=False`` forces it)."""
    lg, gm = _literal(longest), _literal(genomic)
    if (native == 'True' and isinstance(lg, bool) and isinstance(gm, bool) and
            seq_type in ('nucleotide', 'protein')):
        clock = _Clock()
        text, parsed = _gff2fasta_native(genome_sequence, gff, seq_type, order,
                                         longest=lg is True, genomic=gm is True,
                                         from_exons=from_exons == 'True', clock=clock)
        if text is not None:
            _write_bytes(text, b'\n')
            clock.lap('write')
            clock.emit()
            return
        if parsed is not None:
            genome_sequence = parsed  # read once: the object path reuses it
    g = genome.Genome(genome_sequence)
    if from_exons == 'True':
        # reference quirk kept: a str features_to_ignore is a substring test
        g.read_gff(gff, features_to_ignore='CDS', features_to_replace=[('exon', 'CDS')])
    else:
        g.read_gff(gff)
    text = g.annotations.get_fasta('gene', seq_type=seq_type, longest=_literal(longest),
                                   genomic=_literal(genomic), order=order)
    _write(text + '\n')


def _gff2fasta_native(genome_sequence, gff, seq_type, order, longest=False, genomic=False,
                      from_exons=False, clock=None):
    """(text, parsed): the gff2fasta text (bytes) via the native planner, the
    extraction kernel and device text assembly, or (None, GenomeSequence or
    None) when it declines -- the GenomeSequence already parsed, for the
    object path to reuse."""
    if order not in ('py2', 'insertion'):
        raise ValueError("order must be 'insertion' or 'py2'")
    protein = seq_type == 'protein'
    clock = clock or _Clock()

    # The FASTA is read and packed natively (Python reader for unusual
    # headers) on another thread, which starts the device first; this thread
    # reads the GFF meanwhile (read_gff needs no genome), then lowers it
    # against the loaded genome's contigs.  Both native calls release the GIL.
    from concurrent.futures import ThreadPoolExecutor
    fa = genome.read_buffer(genome_sequence)
    clock.lap('fasta_map')

    def load(text):
        clock.at('load_thread_start')
        from . import _lib
        ctx = _lib.default_context()          # device start-up
        clock.at('device_context_ready')
        g = engine.FastaGenome.load(text, ctx=ctx)
        clock.at('genome_on_device')
        return g

    with ThreadPoolExecutor(1) as pool:
        loading = pool.submit(load, fa)
        try:
            read = engine.GffRead.read(genome.read_buffer(gff), from_exons=from_exons)
            clock.lap('gff_read')
        except BaseException:
            # the genome may already be on the device: free it before raising
            try:
                loaded = loading.result()
            except Exception:
                loaded = None
            if loaded is not None:
                loaded.close()
            raise
        try:
            dev = loading.result()
        except BaseException:
            if read is not None:
                read.close()
            raise
        clock.lap('wait_genome')
    owned = dev  # the FastaGenome this call loaded (closed on every return)
    if read is None:  # read_gff takes a diagnostic path: the object path
        if dev is not None:
            dev.close()
        return None, None

    def plan_gff(names, lengths):
        # lowers the one read (None when the lowering takes a diagnostic path)
        return read.lower(names, lengths, protein=protein, order=order, longest=longest,
                          genomic=genomic)

    release = _Release()
    try:
        plan = None
        if dev is not None:
            plan = plan_gff(dev.names, dev.lengths)
            clock.lap('gff_lower')
            if plan is None:
                return None, None
        return _gff2fasta_run(genome_sequence, dev, plan, plan_gff, clock, release)
    finally:
        release.add(read)
        release.add(owned)
        clock.release_thread = release.later()
        clock.lap('close')


def _gff2fasta_run(genome_sequence, dev, plan, plan_gff, clock, release):
    seqs = None
    if dev is None:
        seqs = genome.GenomeSequence(genome_sequence)
        if sum(len(v) for v in seqs.values()) > engine.PART_BASES:
            # several device planes: the object path extracts per plane;
            # decided before anything is packed
            return None, seqs
        dev = seqs.device()
        plan = plan_gff(dev.names, [int(x) for x in dev.lengths])
        if plan is None:
            return None, seqs
    try:
        # records laid out in genome order on the device (neighbouring loci in
        # neighbouring tiles share genome lines: the kernel the bench line
        # times); the device text assembly reads each record at its place, so
        # the text is the record-order text.  longest=True over peptides
        # fetches the payloads for a host render: record order there.
        out = engine.OUT_PEP if plan.protein else engine.OUT_NUC
        ex = engine.ExtractionPlan(dev, plan.exons, plan.txs,
                                   out if plan.n_select else out | engine.OUT_GENOME_ORDER)
        clock.lap('plan_create')
        if plan.n_select:
            # longest=True over peptides: the render picks from the trimmed
            # lengths, on the host
            try:
                return plan.render(*ex.run()), None
            finally:
                ex.close()
        text = engine.FastaText(plan, ex)
        clock.lap('text_create')
        try:
            ex.execute()
            text.execute()  # records + headers + joiners in one device buffer
            ex.sync()
            clock.lap('kernel_and_text_assembly')
            out = text.fetch()
            clock.lap('text_d2h')
            return out, None
        finally:
            release.add(text)
            release.add(ex)
    finally:
        release.add(plan)


def _cds_translate(seq, seg_off):
    """(pep offsets, codon counts, residues) of the segments' frame-0 '+'
    translations (magot_translate_batch, one launch)."""
    from . import _lib
    n = len(seg_off) - 1
    fr = np.zeros(n, np.int32)
    st = np.full(n, ord('+'), np.uint8)
    poff = np.empty(n + 1, dtype=np.uint64)
    codons = np.empty(max(n, 1), dtype=np.int64)
    L = _lib.lib()
    _lib.check(L.magot_translate_sizes(_lib.ptr(seg_off), n, _lib.ptr(fr), _lib.ptr(poff),
                                       _lib.ptr(codons)), 'magot_translate_sizes')
    out = np.empty(max(int(poff[n]), 1), dtype=np.uint8)
    _lib.check(L.magot_translate_batch(_lib.default_context().handle,
                                       _lib.ptr(seq) if len(seq) else None, _lib.ptr(seg_off), n,
                                       _lib.ptr(fr), _lib.ptr(st), None, _lib.ptr(poff),
                                       _lib.ptr(out)), 'magot_translate_batch')
    return poff, codons, out


def _cds2pep_native(data):
    """cds2pep's stdout for a file's bytes: magot_cds_scan (no per-line
    Python), one translation batch, magot_cds_render; None when the line loop
    must run (an empty line's IndexError, a CR inside a line)."""
    from . import _lib
    L = _lib.lib()
    d = engine._text_view(data)
    tp = engine._text_ptr(d)
    n_seg, nb = ctypes.c_uint64(), ctypes.c_uint64()
    rc = L.magot_cds_scan(tp, len(d), ctypes.byref(n_seg), ctypes.byref(nb), None, None, None,
                          None, 0)
    if rc == _lib.ERR_UNSUPPORTED:
        return None
    _lib.check(rc, 'magot_cds_scan')
    n = n_seg.value
    seg_off = np.empty(n + 1, np.uint64)
    hdr_off = np.empty(max(n - 1, 1), np.uint64)
    hdr_len = np.empty(max(n - 1, 1), np.uint64)
    seq = np.empty(max(nb.value, 1), np.uint8)
    _lib.check(L.magot_cds_scan(tp, len(d), ctypes.byref(n_seg), ctypes.byref(nb),
                                _lib.ptr(seg_off), _lib.ptr(hdr_off), _lib.ptr(hdr_len),
                                _lib.ptr(seq), len(seq)), 'magot_cds_scan')
    poff, codons, pep = _cds_translate(seq[:nb.value], seg_off)
    size = ctypes.c_uint64()
    args = (tp, n, _lib.ptr(seg_off), _lib.ptr(hdr_off), _lib.ptr(hdr_len), _lib.ptr(pep),
            _lib.ptr(poff), _lib.ptr(codons))
    _lib.check(L.magot_cds_render(*args, None, 0, ctypes.byref(size)), 'magot_cds_render')
    out = np.empty(max(size.value, 1), np.uint8)
    _lib.check(L.magot_cds_render(*args, _lib.ptr(out), size.value, ctypes.byref(size)),
               'magot_cds_render')
    return out[:size.value]


def cds2pep(fasta_file, native='True'):
    """genome_tools.py:664-675: headers echoed, each record translated; all
    records go to the GPU as one batch.  A file path is scanned natively
    (``native=False`` forces the line loop, which also reproduces the
    reference's IndexError on an empty line)."""
    if not hasattr(fasta_file, 'read'):
        with open(fasta_file, 'rb'):  # the reference open()s the path (:666): a missing file raises
            pass
        if native == 'True' and isinstance(fasta_file, str):
            text = _cds2pep_native(genome.read_buffer(fasta_file))
            if text is not None:
                _write_bytes(text)
                return
    events = []       # ('line', text) | ('pep', job index)
    seqs = []
    failure = None
    work = []
    for raw in genome.ensure_file(fasta_file):
        line = raw.replace('\n', '').replace('\r', '')
        try:
            first = line[0]
        except IndexError as e:
            failure = e
            break
        if first == '>':
            cur = ''.join(work)
            if cur != '':
                events.append(('pep', len(seqs)))
                seqs.append(cur)
                work = []
            events.append(('line', line))
        else:
            work.append(line)
    if failure is None:
        events.append(('pep', len(seqs)))
        seqs.append(''.join(work))
    peps = engine.translate_batch(seqs, [0] * len(seqs), ['+'] * len(seqs)) if seqs else []
    out = []
    for kind, val in events:
        if kind == 'line':
            out.append(val)
        else:
            p = peps[val]
            if p is not None and p[:1] == 'X':
                p = p[1:]
            out.append(str(p))
    _write(''.join(s + '\n' for s in out))
    if failure is not None:
        raise failure


def _gather(seqs, intervals):
    """Bytes of (contig index, start, length, rc) intervals: one kernel launch."""
    if not intervals:
        return []
    ex = np.zeros(len(intervals), dtype=engine.EXON_DTYPE)
    for i, (c, st, ln, rc) in enumerate(intervals):
        ex[i] = ((st | (1 << 63)) if rc else st, c, ln)
    tx = np.zeros(len(intervals), dtype=engine.TX_DTYPE)
    tx['exon_begin'] = np.arange(len(intervals))
    tx['n_exons'] = 1
    nuc, noff, _, _ = engine.extract_records(seqs.device(), ex, tx, engine.OUT_NUC)
    raw = nuc.tobytes().decode('latin-1')
    return [raw[int(noff[i]):int(noff[i + 1])] for i in range(len(intervals))]


def extract_upstream_downstream(genome_sequence, gff, sequence_length, stream,
                                feature_type='gene', namefrom='ID', truncate_names='True',
                                native='True'):
    """genome_tools.py:457-480: the `sequence_length` bases up- or downstream of
    every `feature_type` line, strand-aware.  Reference quirks kept: 'down' on
    '+' and 'up' on '-' are reverse complemented; a strand other than '+'/'-'
    reuses the previous line's sequence (or raises UnboundLocalError); only
    full-length windows print.

    Natively (magot_flank_plan: the GFF scanned in C++, the windows gathered
    by the extraction kernel, the FASTA text assembled on the device) unless
    the input would take one of the reference's error paths, which the line
    loop below reproduces (``native=False`` forces it)."""
    truncate = _literal(truncate_names)
    if native == 'True' and isinstance(truncate, bool):
        text = _flank_native(genome_sequence, gff, sequence_length, stream, feature_type,
                             namefrom, truncate)
        if text is not None:
            _write_bytes(text, b'\n')
            return
    seqs = genome.GenomeSequence(genome_sequence, truncate_names=truncate)
    index = {name: i for i, name in enumerate(seqs)}
    current = None
    items = []
    with open(gff, 'rb') as fh:
        lines = fh.read().decode('latin-1').split('\n')
    lines = [ln + '\n' for ln in lines[:-1]] + ([lines[-1]] if lines[-1] else [])
    for line in lines:
        if line.count('\t') > 5 and line[0] != '#':
            fields = line.split('\t')
            if fields[2] == feature_type:
                name = None
                coords = sorted([int(fields[3]), int(fields[4])])
                for attribute in fields[-1].split(';'):
                    if namefrom == attribute.split('=')[0]:
                        name = attribute.split('=')[1].replace('\r', '').replace('\n', '')
                if name is None:
                    name = 'seq' + str(len(items))
                # evaluation order of the reference: the contig (KeyError),
                # then int(sequence_length) (ValueError)
                if stream == 'up' and fields[6] == '+' or stream == 'down' and fields[6] == '-':
                    stop = coords[0] - 1
                    contig = seqs[fields[0]]
                    n = int(sequence_length)
                    st, ln = genome._slice_interval(contig, stop - n, stop)
                    current = (index[fields[0]], st, ln, False)
                elif stream == 'down' and fields[6] == '+' or stream == 'up' and fields[6] == '-':
                    start = coords[1]
                    contig = seqs[fields[0]]
                    n = int(sequence_length)
                    st, ln = genome._slice_interval(contig, start, start + n)
                    current = (index[fields[0]], st, ln, True)
                if current is None:
                    raise UnboundLocalError(
                        "local variable 'sequence' referenced before assignment")
                if current[2] == int(sequence_length):
                    items.append((name, current))
    texts = _gather(seqs, [iv for _, iv in items])
    _write('\n'.join('>' + name + '\n' + t for (name, _), t in zip(items, texts)) + '\n')


def _flank_native(genome_sequence, gff, sequence_length, stream, feature_type, namefrom,
                  truncate):
    """extract_upstream_downstream's text (bytes, no final newline) via
    magot_flank_plan, one extraction launch and device text assembly; None
    when the FASTA needs the Python reader or the input takes an error path."""
    dev = engine.FastaGenome.load(genome.read_buffer(genome_sequence), truncate_names=truncate)
    if dev is None:
        return None
    plan = engine.GffPlan.flank(genome.read_buffer(gff), dev.names,
                                [int(x) for x in dev.lengths], sequence_length, stream,
                                feature_type=feature_type, namefrom=namefrom)
    if plan is None:
        return None
    try:
        if len(plan.txs) == 0:
            return b''
        ex = engine.ExtractionPlan(dev, plan.exons, plan.txs, engine.OUT_NUC)
        text = engine.FastaText(plan, ex)
        try:
            ex.execute()
            text.execute()
            return text.fetch()
        finally:
            text.close()
            ex.close()
    finally:
        plan.close()


def coords2fasta(fasta_file, seqid, start, stop, truncate_names='False'):
    """genome_tools.py:656-661: header, then contig[start-1:stop] (Python slice
    rules) gathered on the GPU.  The FASTA is read and packed natively
    (magot_genome_load_fasta) unless a header needs the Python reader."""
    _write('>' + seqid + ':' + start + '-' + stop + '\n')
    truncate = _literal(truncate_names)
    dev = None
    if isinstance(truncate, bool):
        dev = engine.FastaGenome.load(genome.read_buffer(fasta_file), truncate_names=truncate)
    if dev is None:
        seqs = genome.Genome(fasta_file, truncate_names=truncate).genome_sequence
        contig = seqs[seqid]
        st, ln = genome._slice_interval(contig, int(start) - 1, int(stop))
        index = {name: i for i, name in enumerate(seqs)}
        _write(_gather(seqs, [(index[seqid], st, ln, False)])[0] + '\n')
        return
    c = dev.index[seqid]  # KeyError, as genome_sequence[seqid]
    a, b = slice(int(start) - 1, int(stop)).indices(int(dev.lengths[c]))[:2]
    _write_bytes(_gather_device(dev, [(c, a, max(0, b - a), False)])[0], b'\n')


def _gather_device(dev, intervals):
    """Bytes of (contig index, start, length, rc) intervals on a device
    genome: one kernel launch."""
    ex = np.zeros(len(intervals), dtype=engine.EXON_DTYPE)
    for i, (c, st, ln, rc) in enumerate(intervals):
        ex[i] = ((st | (1 << 63)) if rc else st, c, ln)
    tx = np.zeros(len(intervals), dtype=engine.TX_DTYPE)
    tx['exon_begin'] = np.arange(len(intervals))
    tx['n_exons'] = 1
    nuc, noff, _, _ = engine.extract_records(dev, ex, tx, engine.OUT_NUC)
    return [nuc[int(noff[i]):int(noff[i + 1])].tobytes() for i in range(len(intervals))]


def _match_fasta(g, order):
    """genome_tools.py:268-271 / 277-280: every match record's get_fasta(),
    joined with newlines and printed; all records gathered in one launch
    (AnnotationSet.get_fasta('match') is that same join).  The match dict is
    built by insertion, never copied: Python-2 order after zero copies."""
    if 'match' not in g.annotations.__dict__:
        raise AttributeError("AnnotationSet instance has no attribute 'match'")
    _write(g.annotations.get_fasta('match', order=order) + '\n')


def blast_csv2fasta(genome_sequence, blast_csv, order='py2'):
    """genome_tools.py:265-271: BLAST -outfmt 10 hits -> subject sequences
    (reverse-complemented where the subject runs backwards)."""
    g = genome.Genome(genome_sequence)
    g.read_blast_csv(blast_csv)
    _match_fasta(g, order)


def exonerate2fasta(genome_sequence, exonerate_file, order='py2'):
    """genome_tools.py:274-280: exonerate vulgar alignments -> the target
    sequence of each alignment's aligned blocks, spliced."""
    g = genome.Genome(genome_sequence)
    g.read_exonerate(exonerate_file)
    _match_fasta(g, order)


def get_seq_from_fasta(genome_sequence, seq_name, truncate_names='False'):
    """genome_tools.py:483-485: one contig as FASTA (host only: a whole
    contig is a copy, not a gather)."""
    g = genome.Genome(genome_sequence, truncate_names=_literal(truncate_names))
    _write(g.get_scaffold_fasta(seq_name) + '\n')


def _dna2orfs_native(fasta_location, from_atg, longest, order):
    """dna2orfs' text (bytes) from the device: the FASTA packed natively, one
    '+' whole-contig record per contig in output order, the six-frame kernel,
    the ORF-calling passes and the text assembly; the host sees the final
    bytes only.  None when the FASTA needs the Python reader, the genome
    exceeds one device plane, or a record is flagged (the reference raises
    there: the loop in dna2orfs reproduces it)."""
    from . import py2order
    dev = engine.FastaGenome.load(genome.read_buffer(fasta_location))
    if dev is None:
        return None
    plan = o6 = calls = None
    try:
        if dev.total_bases > engine.PART_BASES:
            return None
        names = py2order.dict_order(dev.names) if order == 'py2' else list(dev.names)
        if not names:
            return b''
        plan = engine.whole_contig_plan(dev, [dev.index[nm] for nm in names])
        o6 = engine.Orf6Plan(plan)
        o6.execute()
        calls = engine.OrfCalls(o6, from_atg=from_atg, longest=longest)
        if calls.flags().any():
            return None
        return calls.text(names).tobytes()
    finally:
        for obj in (calls, o6, plan, dev):
            if obj is not None:
                obj.close()


def dna2orfs(fasta_location, output_file, from_atg=False, longest=False, order='py2',
             native='True'):
    """genome_tools.py:145-180: every contig translated in six frames, each
    translation split at its stops, one FASTA record per ORF
    ('>contig-pos:P'), or with ``longest`` the longest one per contig
    ('>contig_longestORF'); ``from_atg`` cuts each ORF to 'M' + what follows
    its first M (further Ms removed, as the reference's join does).

    ``from_atg`` and ``longest`` follow the reference's truthiness: from the
    command line every value is a non-empty string, so ``from_atg=False``
    switches it on.  Contigs come in the reference's Python 2 dict order
    unless ``order='insertion'``.

    One deliberate deviation: the reference hands ``translate`` a plain
    ``str`` contig and dies with a TypeError on the first one (SURVEY row
    14); here contigs are Sequences, which is what every other line of the
    function assumes.

    The ORFs are called on the device (engine.OrfCalls).  A contig of <= 4
    bases (translate() is None for frame 2: AttributeError) or, with
    ``longest``, a contig with no non-empty ORF (IndexError), a genome above
    one device plane and a FASTA that needs the Python reader take the loop
    below, which writes what the reference writes up to the failure and
    raises what it raises; ``native=False`` forces it."""
    from_atg, longest = bool(from_atg), bool(longest)
    if order not in ('py2', 'insertion'):
        raise ValueError("order must be 'insertion' or 'py2'")
    if native == 'True' and isinstance(fasta_location, str) and os.path.isfile(fasta_location):
        text = _dna2orfs_native(fasta_location, from_atg, longest, order)
        if text is not None:
            with open(output_file, 'wb') as out:
                out.write(text)
            return
    from . import py2order
    seqs = genome.Genome(fasta_location).genome_sequence
    names = py2order.dict_order(list(seqs)) if order == 'py2' else list(seqs)
    with open(output_file, 'wb') as out:
        batch, bases = [], 0
        for i, name in enumerate(names):
            batch.append(name)
            bases += len(seqs[name])
            if bases < (1 << 28) and i + 1 < len(names):
                continue
            sixes = engine.orf6_batch([seqs[nm] for nm in batch])  # one launch per batch
            for nm, six in zip(batch, sixes):
                _dna2orfs_contig(out, nm, len(seqs[nm]), six, from_atg, longest)
            batch, bases = [], 0


def _dna2orfs_contig(out, name, length, six, from_atg, longest):
    """genome_tools.py:152-179 for one contig from its six translations (loop
    order: frame 0, 1, 2 x strand '-', '+')."""
    candidates, best = [], 0
    for j, translated in enumerate(six):
        frame, plus = j >> 1, j & 1
        if translated is None:
            raise AttributeError("'NoneType' object has no attribute 'split'")
        pos = frame if plus else length - frame
        for orf in translated.split('*'):
            start = pos
            pos += (1 + len(orf)) * 3
            output_orf = 'M' + ''.join(orf.split('M')[1:]) if from_atg else orf
            if longest:
                if len(output_orf) > best:
                    candidates.append('>' + name + '_longestORF\n' + output_orf + '\n')
                    best = len(output_orf)
            else:
                out.write(('>' + name + '-pos:' + str(start) + '\n' + output_orf +
                           '\n').encode('latin-1'))
    if longest:
        out.write(candidates[-1].encode('latin-1'))


_CDSPEP_INT = re.compile(r'\s*[+-]?[0-9]+\s*\Z')


def get_CDS_peptides(genome_sequence, gff, output_location, gene_name_filters=[],
                     gene_length_filter=None, names_from='CDS', order='py2', native='True'):
    """genome_tools.py:283-321: for every CDS feature of every kept gene, the
    longest six-frame ORF of that CDS ('>name\\nORF\\n'), the exon peptides that
    prep4apollo maps with tblastn.

    One deliberate deviation: the reference calls ``Genome.read_gff3``, which
    does not exist, and dies there; here it is ``read_gff``,
    with which the rest of the function runs.

    A gene is dropped when an element of ``gene_name_filters`` is a substring
    of its ID (from the command line the argument is a string, and every
    character is a filter, as in the reference), or when ``gene_length_filter``
    is given and the first record of its ``get_fasta()`` is shorter.
    ``names_from``: 'CDS' (the CDS's ID), 'transcript' or 'gene' (that ID +
    '-CDS' + n).  Genes come in the reference's Python 2 dict order unless
    ``order='insertion'``.

    On the device (engine.LongestOrfs over one extraction plan, one record per
    printed CDS) when the host planner can lower the annotation; a CDS without
    any ORF (IndexError in the reference) is found from the kernel's flags, and
    the file holds what the reference had written before it.  Every other way
    the reference leaves the straight path, and ``native=False``, take the
    object path, which restates the reference.  Nothing is written before the
    path is known.  ``get_CDS_peptides.last_path`` names the path the last call
    took."""
    if order not in ('py2', 'insertion'):
        raise ValueError("order must be 'py2' or 'insertion'")
    filters = list(gene_name_filters)
    result = None
    if native != 'True':
        why = "native != 'True'"
    elif names_from not in ('CDS', 'transcript', 'gene'):
        why = 'invalid names_from'
    elif not all(isinstance(f, str) for f in filters):
        why = 'a filter that is not a string'
    elif not (gene_length_filter is None or type(gene_length_filter) is int or
              (isinstance(gene_length_filter, str) and _CDSPEP_INT.match(gene_length_filter))):
        why = 'bad integer'
    elif not all(isinstance(p, str) and os.path.isfile(p) for p in (genome_sequence, gff)):
        why = 'not a regular file'
    else:
        glf = None if gene_length_filter is None else int(gene_length_filter)
        if glf is not None and abs(glf) >= 1 << 62:
            why = 'bad integer'
        else:
            result, why = _cds_peptides_native(genome_sequence, gff, filters, glf, names_from, order)
    if result is not None:
        get_CDS_peptides.last_path = ('get_CDS_peptides', 'native', None)
        text, failed = result
        with open(output_location, 'wb') as out:
            out.write(text)
        if failed:
            raise IndexError('list index out of range')
        return
    get_CDS_peptides.last_path = ('get_CDS_peptides', 'host', why)
    _cds_peptides_host(genome_sequence, gff, output_location, filters, gene_length_filter,
                       names_from, order)


get_CDS_peptides.last_path = None


def _cds_peptides_native(genome_sequence, gff, filters, glf, names_from, order):
    """((text bytes, whether the reference raises IndexError behind it), None),
    or (None, why) where the planner or the device path declines."""
    dev = engine.FastaGenome.load(genome.read_buffer(genome_sequence))
    if dev is None:
        return None, 'the FASTA needs the Python reader'
    read = ex = calls = None
    try:
        if dev.total_bases > engine.PART_BASES:
            return None, 'a genome above one device plane'
        read = engine.GffRead.read(genome.read_buffer(gff))
        if read is None:
            return None, 'read_gff takes a diagnostic path'
        plan = read.lower_cds(dev.names, dev.lengths, filters, glf, names_from, order)
        if plan is None:
            return None, 'the annotation takes a diagnostic path'
        if not plan.n_records:
            return (b'', False), None
        ex = engine.ExtractionPlan(dev, plan.exons, plan.txs,
                                   engine.OUT_NUC | engine.OUT_GENOME_ORDER)
        ex.execute()
        calls = engine.LongestOrfs(ex)
        flagged = np.flatnonzero(calls.flags())
        n_print = plan.n_records
        if len(flagged):
            # the reference computes every ORF of a transcript before it writes
            # the first: the output ends where the failing record's group begins
            g = int(np.searchsorted(plan.group_off, flagged[0], side='right')) - 1
            n_print = int(plan.group_off[g])
        text = calls.text_blob(plan.names, plan.name_off, n_print).tobytes()
        return (text, bool(len(flagged))), None
    finally:
        for obj in (calls, ex, read, dev):
            if obj is not None:
                obj.close()


def _cds_peptides_host(genome_sequence, gff, output_location, filters, gene_length_filter,
                       names_from, order):
    """The reference's loop over the annotation objects.  The walk collects
    every CDS sequence up to the first exception, one six-frame launch
    translates them all, and the replay writes what the reference writes and
    raises what it raises, in its order.

    One difference, on stdout only: the walk does not know yet which CDS has no
    ORF, so it goes on past one that will raise IndexError, and a diagnostic
    that ``get_seq()`` or ``get_fasta()`` prints for a later gene (a seqid the
    genome does not have, say) is printed although the reference had raised
    before it.  The exception and the file are the reference's."""
    g = genome.Genome(genome_sequence)
    g.read_gff(gff)
    ann = g.annotations
    genes = list(ann.gene)
    if order == 'py2':
        genes = genome.order_after_copies(genes, ann.__dict__.get('_magot_copies', 0))
    work = []       # per transcript: [gene ID, ID, strand, {coords: (CDS ID, seq index)}, seqs, whole]
    pending = None  # the exception the walk met: raised behind what precedes it
    try:
        for gene in genes:
            gene_obj = ann.gene[gene]
            keepgene = True
            for name_filter in filters:
                if name_filter in gene_obj.ID:
                    keepgene = False
            if gene_length_filter != None:  # noqa: E711
                seqlen = len(gene_obj.get_fasta().split('\n')[1])
                if isinstance(gene_length_filter, str) and '_' in gene_length_filter:
                    raise ValueError("invalid literal for int() with base 10: %r"
                                     % gene_length_filter)
                if seqlen < int(gene_length_filter):
                    keepgene = False
            if keepgene:
                for transcript in gene_obj.child_list:
                    transcript_obj = ann.transcript[transcript]
                    entry = [gene_obj.ID, transcript_obj.ID, transcript_obj.strand, {}, [], False]
                    work.append(entry)
                    for CDS in transcript_obj.child_list:
                        CDS_obj = ann.CDS[CDS]
                        seq = CDS_obj.get_seq()
                        if seq is None:
                            raise AttributeError("'NoneType' object has no attribute 'get_orfs'")
                        entry[3][CDS_obj.coords] = (CDS_obj.ID, len(entry[4]))
                        entry[4].append(str(seq))
                    entry[5] = True
    except Exception as e:  # noqa: BLE001
        pending = e
    seqs = [s for entry in work for s in entry[4]]
    sixes = engine.orf6_batch(seqs) if seqs else []
    at = 0
    with open(output_location, 'wb') as out:
        for gene_id, transcript_id, strand, CDSdict, tseqs, whole in work:
            orfs = [genome._orfs_from_translations(sixes[at + i], True, False)
                    for i in range(len(tseqs))]  # IndexError: no candidate
            at += len(tseqs)
            if not whole:
                break
            CDSlist = sorted(CDSdict)
            if strand == "-":
                CDSlist.reverse()
            counter = 1
            for CDS in CDSlist:
                if names_from == 'CDS':
                    pep_name = CDSdict[CDS][0]
                elif names_from == 'transcript':
                    pep_name = transcript_id + '-CDS' + str(counter)
                    counter = counter + 1
                elif names_from == 'gene':
                    pep_name = gene_id + '-CDS' + str(counter)
                    counter = counter + 1
                else:
                    _write("invalid option for 'names_from' argument\n")
                    break
                out.write(('>' + pep_name + '\n' + orfs[CDSdict[CDS][1]] + '\n').encode('latin-1'))
    if pending is not None:
        raise pending


_MASK_OVERWRITE = ('True', 'T', 'true', 't', 'TRUE')
_MASK_KEEP = ('False', 'F', 'false', 'f', 'FALSE')
_PY_SPACE = b' \t\n\r\x0b\x0c'


def _py2_int(field):
    """int() of a byte string as Python 2 reads it: surrounding whitespace,
    one optional sign, decimal digits (no '_' separators)."""
    s = field.strip(_PY_SPACE)
    digits = s[1:] if s[:1] in (b'+', b'-') else s
    if not digits or not digits.isdigit():
        raise ValueError('invalid literal for int() with base 10: %r' % field.decode('latin-1'))
    return int(s)


def _file_lines(path):
    """``for line in open(path)`` of Python 2: lines end after '\\n' only."""
    return _lines_of(genome.read_buffer(path))


def _lines_of(data):
    """The same over a buffer."""
    lines = bytes(data).split(b'\n')
    return [ln + b'\n' for ln in lines[:-1]] + ([lines[-1]] if lines[-1] else [])


def _mask_native(genome_sequence, gff, hard, keep_case, feature_type, order, clock):
    """mask_from_gff's text (a uint8 array) from the device: the FASTA packed
    natively, the GFF scanned by magot_mask_plan, every contig gathered whole
    in output order, the coverage paint and the text pass; one D2H.  None
    when only the reference's sequential loop is exact (engine.MaskPlan,
    engine.mask_fasta_check) or the genome exceeds one device plane."""
    from . import py2order
    fa = genome.read_buffer(genome_sequence)
    dev = engine.FastaGenome.load(fa, truncate_names=True)
    clock.lap('fasta_read')
    if dev is None:
        return None
    plan = ex = mask = None
    try:
        if (not dev.names or dev.total_bases > engine.PART_BASES or
                not engine.mask_fasta_check(fa, len(dev.names))):
            return None
        plan = engine.MaskPlan.build(genome.read_buffer(gff), dev.names,
                                     [int(x) for x in dev.lengths], feature_type=feature_type,
                                     hard=hard, keep_case=keep_case)
        clock.lap('gff_scan')
        if plan is None:
            return None
        names = py2order.dict_order(dev.names) if order == 'py2' else list(dev.names)
        idx = [dev.index[nm] for nm in names]
        ex = engine.whole_contig_plan(dev, idx)
        mask = engine.GenomeMask(ex, plan, idx, names)
        clock.lap('plan_create')
        ex.execute()
        mask.execute()
        ex.sync()
        clock.lap('kernels')
        out = mask.fetch()
        clock.lap('text_d2h')
        return out
    finally:
        for obj in (mask, ex, plan, dev):
            if obj is not None:
                obj.close()


def mask_from_gff(genome_sequence, gff, mask_type='soft', overwrite_softmask='True',
                  feature_type='CDS', order='py2', native='True'):
    """genome_tools.py:394-428: the genome with every base under a
    ``feature_type`` line of the GFF lower-cased (``mask_type='soft'``) or
    replaced by 'N' ('hard'), after the whole genome was upper-cased
    (``overwrite_softmask`` 'True') or as it is ('False'); one
    '>name\\nsequence\\n' record per contig, the sequence on one line.  Names
    are cut at the first whitespace; contigs come in the reference's Python 2
    dict order unless ``order='insertion'``.

    On the device (engine.GenomeMask: a coverage plane painted from the
    interval table, one text pass) whenever the features only decide "covered
    or not" per base.  Everything whose result depends on the reference
    replaying the features one after another on Python lists -- a negative
    slice index (start < 1), a hard mask reaching past its contig (the list
    changes length and shifts every later feature), its exceptions (KeyError,
    ValueError), its two invalid-argument messages, and FASTA files whose
    contigs the native reader sees differently (empty or repeated contigs,
    '> name' headers, sequence before the first header) -- takes the line loop
    below, which restates the reference; ``native=False`` forces it."""
    if order not in ('py2', 'insertion'):
        raise ValueError("order must be 'insertion' or 'py2'")
    if (native == 'True' and mask_type in ('soft', 'hard') and
            overwrite_softmask in _MASK_OVERWRITE + _MASK_KEEP and
            isinstance(genome_sequence, str) and isinstance(gff, str)):
        clock = _Clock()
        text = _mask_native(genome_sequence, gff, mask_type == 'hard',
                            overwrite_softmask in _MASK_KEEP, feature_type, order, clock)
        if text is not None:
            _write_bytes(text)
            clock.lap('write')
            clock.emit()
            return
    from . import py2order
    genome_dict = {}
    working_seqid = ''
    for line in _file_lines(genome_sequence):
        if line[:1] == b'>':
            working_seqid = line.split()[0][1:].decode('latin-1')
            genome_dict[working_seqid] = bytearray()
        else:
            seq = line.replace(b'\r', b'').replace(b'\n', b'')
            if overwrite_softmask in _MASK_OVERWRITE:
                genome_dict[working_seqid].extend(seq.upper())  # ASCII only, as Python 2's
            elif overwrite_softmask in _MASK_KEEP:
                genome_dict[working_seqid].extend(seq)
            else:
                _write("Invalid option for 'overwrite_softmask', argument accepts 'True' or "
                       "'False'\n")
                return
    for line in _file_lines(gff):
        if line.count(b'\t') > 5:
            fields = line.split(b'\t')
            if fields[2].decode('latin-1') == feature_type:
                start = _py2_int(fields[3])
                stop = _py2_int(fields[4])
                if mask_type == 'soft':
                    contig = genome_dict[fields[0].decode('latin-1')]
                    contig[start - 1:stop] = contig[start - 1:stop].lower()
                elif mask_type == 'hard':
                    # a replacement of another length moves every later base
                    contig = genome_dict[fields[0].decode('latin-1')]
                    contig[start - 1:stop] = b'N' * max(0, 1 + stop - start)
                else:
                    _write("Invalid option for mask_type, argument accepts 'soft' and 'hard'\n")
                    return
    names = py2order.dict_order(list(genome_dict)) if order == 'py2' else list(genome_dict)
    parts = []
    for name in names:
        parts += [b'>', name.encode('latin-1'), b'\n', bytes(genome_dict[name]), b'\n']
    _write_bytes(*parts)


def _at_content_native(fasta, clock):
    """at_content_from_fasta's text (bytes) from the device: the FASTA packed
    natively under its whole header lines, the A/T and the C/G class of every
    base as bit tracks, one count per contig of each.  None where the line
    loop sees other records than the native reader: a file that does not
    start with a header, a '>' inside a line or an empty record (the file's
    '>' bytes are then not one per contig), a repeated name, or a genome above
    one device plane."""
    fa = genome.read_buffer(fasta)
    if bytes(fa[:1]) != b'>':
        return None
    dev = engine.FastaGenome.load(fa, truncate_names=False)
    clock.lap('fasta_read')
    if dev is None:
        return None
    track = None
    try:
        n = len(dev.names)
        if (n == 0 or dev.total_bases > engine.PART_BASES or len(set(dev.names)) != n or
                int(np.count_nonzero(np.frombuffer(fa, dtype=np.uint8) == 62)) != n):
            return None
        clock.lap('header_check')
        track = engine.GenomeTrack(dev)
        whole = (np.arange(n), np.zeros(n, np.int64), [int(x) for x in dev.lengths])
        track.base_class(gc=False, replace=True)
        ats = track.count(*whole)
        track.base_class(gc=True, replace=True)
        gcs = track.count(*whole)
        clock.lap('kernels')
        return b''.join(b'%s\t%d\t%d\n' % (nm.encode('latin-1'), a, g)
                        for nm, a, g in zip(dev.names, ats.tolist(), gcs.tolist()))
    finally:
        for obj in (track, dev):
            if obj is not None:
                obj.close()


def at_content_from_fasta(fasta, native='True'):
    """genome_tools.py:506-524: ``name \\t ATs \\t GCs`` per record, counted
    without regard to case; the name is the header line without '>' and its
    line end.  On the device (engine.GenomeTrack: the base-class pass and the
    count pass) for a FASTA file whose records the native reader sees as the
    reference's line loop does; otherwise, and with ``native=False``, the line
    loop below, which restates the reference and raises what it raises (a
    file that starts with sequence: UnboundLocalError)."""
    if native == 'True' and isinstance(fasta, str) and os.path.isfile(fasta):
        clock = _Clock()
        text = _at_content_native(fasta, clock)
        if text is not None:
            _write_bytes(text)
            clock.lap('write')
            clock.emit()
            return
    firstline = True
    out = []
    with open(fasta, 'rb') as fh:
        lines = fh.read().split(b'\n')
    lines = [ln + b'\n' for ln in lines[:-1]] + ([lines[-1]] if lines[-1] else [])
    try:
        for line in lines:
            if line == b'\n':
                continue
            elif b'>' in line:
                if firstline:
                    firstline = False
                else:
                    out.append(name + b'%d\t%d\n' % (ats, gcs))
                name = line[1:].replace(b'\n', b'').replace(b'\r', b'') + b'\t'
                ats = 0
                gcs = 0
            else:
                up = line.upper()  # ASCII only, as Python 2's
                ats = ats + up.count(b'A') + up.count(b'T')
                gcs = gcs + up.count(b'G') + up.count(b'C')
        out.append(name + b'%d\t%d\n' % (ats, gcs))
    finally:
        _write_bytes(*out)  # what was printed before an exception stays printed


class _DepthDecline(Exception):
    """Why depth_from_gff leaves a call to its host loop."""


def _depth_order(table, aset, order):
    """The iteration order of one of the annotation set's tables."""
    from . import py2order
    keys = list(table)
    if order == 'py2':
        keys = py2order.order_after_copies(keys, aset.__dict__.get('_magot_copies', 0))
    return keys


def _depth_features(features):
    """``eval(features)`` for literals (nothing is executed here); a bare
    word is a NameError, as it is there."""
    try:
        return ast.literal_eval(features)
    except ValueError:
        raise NameError('name %r is not defined' % features)


def _depth_native(depth_file, aset, features_list, stream_length, order, clock):
    """depth_from_gff's text (a list of bytes) with every sum from the device
    (engine.DepthTrack); raises _DepthDecline with the reason otherwise."""
    from . import py2order
    if not (isinstance(features_list, (list, tuple, set, frozenset)) and
            all(isinstance(f, str) for f in features_list)):
        raise _DepthDecline('features is not a container of strings')
    try:
        L = _py2_int(stream_length.encode('latin-1'))
    except (ValueError, AttributeError, UnicodeEncodeError):
        raise _DepthDecline('stream_length is not an integer')
    if L < 0:
        raise _DepthDecline('stream_length < 0: a negative slice bound')
    if aset is None or not isinstance(aset.__dict__.get('CDS'), dict) or not aset.CDS:
        raise _DepthDecline('no CDS')
    want_cds, want_up = 'CDS' in features_list, 'upstream' in features_list
    cds_ids = _depth_order(aset.CDS, aset, order)
    try:
        table = aset.__dict__[aset[aset.CDS[cds_ids[0]].parent].feature_type]
    except (KeyError, TypeError, AttributeError):
        raise _DepthDecline("the first CDS's parent is not in the set")
    track = engine.DepthTrack.parse(genome.read_buffer(depth_file))
    clock.lap('depth_parse')
    try:
        if track.declined is not None:
            raise _DepthDecline('depth file: %s at line %s' % track.declined)
        lengths = track.lengths.tolist()

        def clip(seqid, a, b):
            """(contig, start, length) of arr[a:b], or None for a missing contig"""
            c = track.index.get(seqid)
            if c is None:
                return None
            lo, hi = slice(a, b).indices(lengths[c])[:2]
            return (c, lo, max(0, hi - lo))

        # CDS rows, sorted by parent: the device sums them per row and per parent
        cds_rows, parents, member = [], [], {}
        if want_cds:
            for cid in cds_ids:
                cds = aset.CDS[cid]
                if not isinstance(cds.parent, str):
                    raise _DepthDecline('a CDS without a parent')
                if not (isinstance(cds.coords[0], int) and isinstance(cds.coords[1], int)):
                    raise _DepthDecline('a coordinate is not an integer')
                if cds.coords[0] < 1 or cds.coords[1] < 0:
                    raise _DepthDecline('a CDS start < 1 or end < 0: a negative slice bound')
                if cds.parent not in member:
                    member[cds.parent] = []
                    parents.append(cds.parent)
                row = clip(cds.seqid, cds.coords[0] - 1, cds.coords[1])
                member[cds.parent].append(len(cds_rows))
                cds_rows.append((row, cds.parent, cds.seqid))
            if cds_rows[0][0] is None:
                raise _DepthDecline('the first CDS is on a contig missing from the depth file')
        up_rows = []
        if want_up:
            for tid in _depth_order(table, aset, order):
                tx = table[tid]
                if tx.strand not in ('+', '-'):
                    raise _DepthDecline("a transcript strand other than '+' / '-'")
                try:
                    lo, hi = tx.get_coords()
                except Exception:
                    raise _DepthDecline('a transcript without coordinates')
                if not (isinstance(lo, int) and isinstance(hi, int)):
                    raise _DepthDecline('a coordinate is not an integer')
                if lo < 1 or hi < 0:
                    raise _DepthDecline('a transcript start < 1 or end < 0: a negative slice bound')
                if not isinstance(tid, str) or not isinstance(tx.seqid, str):
                    raise _DepthDecline('a transcript without a name')
                if tx.strand == '+':
                    row = clip(tx.seqid, max(0, lo - 1 - L), lo - 1)
                else:
                    row = clip(tx.seqid, hi, hi + L)
                up_rows.append((row, tid, tx.seqid))
            if not want_cds and up_rows and up_rows[0][0] is None:
                raise _DepthDecline('the first transcript is on a contig missing from the depth file')
        clock.lap('rows')

        # device rows: the present CDS rows parent by parent, then the flanks
        rows, offsets, cds_at = [], [0], {}
        for parent in parents:
            for k in member[parent]:
                if cds_rows[k][0] is not None:
                    cds_at[k] = len(rows)
                    rows.append(cds_rows[k][0])
            offsets.append(len(rows))
        up_at = {}
        for k, (row, _, _) in enumerate(up_rows):
            if row is not None:
                up_at[k] = len(rows)
                rows.append(row)
        if rows:
            tab = np.array(rows, dtype=np.int64).reshape(-1, 3)
            sums, groups = track.group_sums(tab[:, 0], tab[:, 1], tab[:, 2], offsets)
            sums, groups = sums.tolist(), groups.tolist()
        else:
            sums, groups = [], [0] * len(parents)
        clock.lap('kernels')
    finally:
        track.close()

    # the reference's carry-over: a feature on a missing contig adds the sum
    # before it once more
    out, missing, covsum = [], [], None
    if want_cds:
        out.append(b'#CDS counts\n')
        total = dict(zip(parents, groups))
        for k, (row, parent, seqid) in enumerate(cds_rows):
            if row is not None:
                covsum = sums[cds_at[k]]
            else:
                missing.append(parent + ' on ' + seqid)
                total[parent] += covsum
        shown = py2order.dict_order(parents) if order == 'py2' else parents
        out += [('%s\t%d\n' % (parent, total[parent])).encode('latin-1') for parent in shown]
    if want_up:
        out.append(b'#upstream ' + stream_length.encode('latin-1') + b'bp counts\n')
        for k, (row, tid, seqid) in enumerate(up_rows):
            if row is not None:
                covsum = sums[up_at[k]]
            else:
                missing.append(tid + ' on ' + seqid)
            out.append(('%s\t%d\n' % (tid, covsum)).encode('latin-1'))
    out += _depth_missing(missing, order)
    return out


def _depth_missing(missing, order):
    """genome_tools.py:649-652: ``list(set(missing_list))``."""
    from . import py2order
    if not missing:
        return []
    seen = list(dict.fromkeys(missing))
    if order == 'py2':
        seen = py2order.dict_order(seen)
    return [b'#missing from depth file\n'] + [(m + '\n').encode('latin-1') for m in seen]


def _depth_host(depth_file, aset, features_list, stream_length, order, out):
    """genome_tools.py:602-652 line for line; what it prints goes to ``out``."""
    from . import py2order
    missing = []
    lines = _file_lines(depth_file)
    lens = {}
    for line in lines:
        seqid = line.split()[0]
        if seqid in lens:
            lens[seqid] = lens[seqid] + 1
        else:
            lens[seqid] = 1
    arrays = {}
    for seqid in lens:
        arrays[seqid.decode('latin-1')] = np.zeros(lens[seqid], dtype=np.int64)
    for line in lines:
        fields = line.split()
        if len(fields) > 1:
            value = _py2_int(fields[2])
            arrays[fields[0].decode('latin-1')][_py2_int(fields[1]) - 1] = value
    unbound = UnboundLocalError("local variable 'covsum' referenced before assignment")
    covsum = None
    if 'CDS' in features_list:
        out.append(b'#CDS counts\n')
        totals = {}
        for cid in _depth_order(aset.CDS, aset, order):
            cds = aset.CDS[cid]
            if cds.seqid in arrays:
                covsum = int(arrays[cds.seqid][cds.coords[0] - 1:cds.coords[1]].sum())
            else:
                missing.append(cds.parent + ' on ' + cds.seqid)
            if covsum is None:
                raise unbound
            if cds.parent in totals:
                totals[cds.parent] = totals[cds.parent] + covsum
            else:
                totals[cds.parent] = covsum
        shown = py2order.dict_order(list(totals)) if order == 'py2' else list(totals)
        for parent in shown:
            out.append((parent + '\t' + str(totals[parent]) + '\n').encode('latin-1'))
    if 'upstream' in features_list:
        out.append(('#upstream ' + stream_length + 'bp counts\n').encode('latin-1'))
        first = _depth_order(aset.CDS, aset, order)[0]
        table = aset.__dict__[aset[aset.CDS[first].parent].feature_type]
        start = stop = None
        for tid in _depth_order(table, aset, order):
            tx = table[tid]
            if tx.strand == '+':
                stop = tx.get_coords()[0] - 1
                start = stop - _py2_int(stream_length.encode('latin-1'))
                if start < 0:
                    start = 0
            elif tx.strand == '-':
                start = tx.get_coords()[1]
                stop = start + _py2_int(stream_length.encode('latin-1'))
            if tx.seqid in arrays:
                if start is None:
                    raise UnboundLocalError("local variable 'start' referenced before assignment")
                covsum = int(arrays[tx.seqid][start:stop].sum())
            else:
                missing.append(tid + ' on ' + tx.seqid)
            if covsum is None:
                raise unbound
            out.append((tid + '\t' + str(covsum) + '\n').encode('latin-1'))
    out += _depth_missing(missing, order)


def depth_from_gff(depth_file, gff, features="['CDS','intron','upstream','downstream']",
                   stream_length='1000', order='py2', native='True'):
    """genome_tools.py:598-652: from a ``samtools depth`` table (``seqid \\t
    position \\t depth``, one line per base) and a GFF, the summed depth under
    every transcript's CDS ('CDS' in ``features``) and over the
    ``stream_length`` bases upstream of every transcript ('upstream'), then
    the features whose contig the table lacks.  'intron' and 'downstream' do
    nothing, as in the reference.  Reference quirks kept: a contig's array has
    as many slots as the table has lines for it; a feature on a missing contig
    repeats (a CDS: adds once more) the sum before it.

    On the device (engine.DepthTrack: the table parsed into an int32 per line
    chunk by chunk, a sum directory, one sum per CDS and flank and one total
    per transcript) when the table is inside the native grammar -- every
    contig one run of lines with positions 1, 2, .. -- and no feature makes
    the reference wrap a slice or raise: a start < 1, an end < 0, a negative
    ``stream_length``, a strand other than '+'/'-', a first feature on a
    missing contig, no CDS, ``features`` that is no container of strings.
    Everything else, and ``native=False``, takes the host loop, which restates
    the reference and raises what it raises; what was printed before stays
    printed.  ``depth_from_gff.last_path`` names the path the last call took
    and why.

    Tables come in the reference's Python 2 dict order unless
    ``order='insertion'``.  The lines after '#missing from depth file' are a
    Python 2 *set's*: py2order.dict_order over the first occurrences is
    believed to model it (CPython 2.7's setobject.c uses the same hash, probe
    sequence and growth rule as its dict), but no Python 2 has been run to
    confirm it."""
    if order not in ('py2', 'insertion'):
        raise ValueError("order must be 'insertion' or 'py2'")
    clock = _Clock()
    aset = genome.read_gff(gff)
    clock.lap('gff_read')
    depth_from_gff.last_path = ('depth_from_gff', 'host', 'features is not a literal')
    features_list = _depth_features(features)
    why = "native != 'True'"
    if native == 'True' and isinstance(depth_file, str) and os.path.isfile(depth_file):
        try:
            out = _depth_native(depth_file, aset, features_list, stream_length, order, clock)
            depth_from_gff.last_path = ('depth_from_gff', 'native', None)
            _write_bytes(*out)
            clock.lap('write')
            clock.emit()
            return
        except _DepthDecline as e:
            why = str(e)
    depth_from_gff.last_path = ('depth_from_gff', 'host', why)
    out = []
    try:
        _depth_host(depth_file, aset, features_list, stream_length, order, out)
    finally:
        _write_bytes(*out)  # what was printed before an exception stays printed


depth_from_gff.last_path = None


def _fqstats_host(fastq_location):
    """fqstats' figures from a line loop on the host, as ReadLengths.stats()
    gives them."""
    lengths = []
    with open(fastq_location, 'rb') as fh:
        for k, line in enumerate(fh):  # binary: a line ends at LF only
            if k % 4 == 1:
                lengths.append(len(line) - 1)
    reads, bases = len(lengths), sum(lengths)
    mean = bases // reads  # no reads: ZeroDivisionError, as there
    lengths.sort(reverse=True)
    marks = [None, None, None]
    running = 0
    for length in lengths:
        running += length
        for k, mark in enumerate((bases // 4, bases // 2, bases * 3 // 4)):
            if marks[k] is None and running > mark:
                marks[k] = length
    return {'reads': reads, 'bases': bases, 'mean': mean, 'median': lengths[reads // 2],
            'reads25': lengths[reads // 4], 'reads75': lengths[reads * 3 // 4],
            'n25': marks[0], 'n50': marks[1], 'n75': marks[2]}


def _fqstats_native(fastq_location, clock):
    import mmap
    with open(fastq_location, 'rb') as fh:
        try:
            size = os.fstat(fh.fileno()).st_size
            data = mmap.mmap(fh.fileno(), 0, access=mmap.ACCESS_READ) if size else b''
        except (ValueError, OSError):  # not a file that maps: a pipe, a device
            data = fh.read()
    clock.lap('open')
    lengths = engine.ReadLengths.parse(data)
    try:
        clock.lap('kernels')
        return lengths.stats()
    finally:
        lengths.close()


def fqstats(fastq_location, native='True'):
    """genome_tools.py:85-124: read count, total bases, median and mean
    length, the lengths a quarter and three quarters of the way down the
    descending list, and N25 / N50 / N75 of a FASTQ file.  Every fourth line
    from the second is a read, whatever it holds; lines end at LF only and a
    read's length is its line without the LF (a CR counts; a last line without
    LF counts one short, as there).  Python 2 integers: every division
    floors.  An N-value never set (no bases at all) prints ``False``; a file
    without reads raises ZeroDivisionError before anything is printed; a
    missing file raises OSError.

    On the device (engine.ReadLengths: the file streamed in chunks cut
    anywhere, a line index from LF counts, the lengths as a histogram and the
    figures reduced from it) for every file; ``native=False`` takes a line
    loop on the host instead, for that switch and for timing.
    ``fqstats.last_path`` names the path the last call took."""
    clock = _Clock()
    if native == 'True':
        fqstats.last_path = ('fqstats', 'native', None)
        s = _fqstats_native(fastq_location, clock)
        if not s['reads']:
            raise ZeroDivisionError('integer division or modulo by zero')
        s['mean'] = s['bases'] // s['reads']
    else:
        fqstats.last_path = ('fqstats', 'host', "native != 'True'")
        s = _fqstats_host(fastq_location)
    n_value = lambda v: 'False' if v is None else str(v)  # noqa: E731
    _write(''.join([
        '%d reads\n' % s['reads'],
        'total basepairs=%d\n' % s['bases'],
        'median length=%d\n' % s['median'],
        'mean length=%d\n' % s['mean'],
        '25%% of reads >%d\n' % s['reads25'],
        '75%% of reads >%d\n' % s['reads75'],
        'n25=' + n_value(s['n25']) + '\n',
        'n50=' + n_value(s['n50']) + '\n',
        'n75=' + n_value(s['n75']) + '\n']))
    clock.lap('write')
    clock.emit()


fqstats.last_path = None


def _map_file(path):
    """The bytes of the file at ``path`` (``open(path)`` of the reference: a
    missing file raises), memory-mapped where it can be."""
    import mmap
    with open(path, 'rb') as fh:
        try:
            size = os.fstat(fh.fileno()).st_size
            return mmap.mmap(fh.fileno(), 0, access=mmap.ACCESS_READ) if size else b''
        except (ValueError, OSError):  # not a file that maps: a pipe, a device
            return fh.read()


def _purge_host(first, second, out):
    """The reference's loops restated; kept lines are appended to ``out`` as
    they would be printed, so what came before an exception is there."""
    purge_dict = {}
    for line in _lines_of(first):
        if line.count(b'\t') > 6:
            x = line.split(b'\t')
            coords = [_py2_int(x[3]), _py2_int(x[4])]
            purge_dict.setdefault(x[0], []).append(coords)
    for line in _lines_of(second):
        printline = True
        if line.count(b'\t') > 6:
            x = line.split(b'\t')
            if x[0] in purge_dict:
                c0, c1 = _py2_int(x[3]), _py2_int(x[4])
                for p0, p1 in purge_dict[x[0]]:
                    if p0 < c0 < p1 or p0 < c1 < p1 or c0 < p0 < c1:
                        printline = False
                        break  # the reference goes on; nothing can set it back
            if printline:  # inside the test for tabs: other lines are never printed
                out.append(line[:-1] + b'\n')


def _purge_native(first, second, clock):
    """(purge_overlaps' text as a uint8 array, None) from the device: both
    texts lowered by magot_overlap_plan, the first file's intervals sorted into
    an engine.IntervalIndex, one purge query per line of the second file that
    has a known seqid, the kept lines copied on the host.  (None, reason) when
    only the reference's sequential run is exact."""
    plan, why = engine.OverlapPlan.build(first, second)
    clock.lap('gff_scan')
    if plan is None:
        return None, why
    index = None
    try:
        t0, t1 = plan.tables
        rows = np.flatnonzero(t0['flag'])
        index = engine.IntervalIndex(t0['seq'][rows], t0['c0'][rows], t0['c1'][rows],
                                     n_seq=plan.n_seq)
        clock.lap('index')
        asked = np.flatnonzero(t1['seq'] != engine._lib.OVERLAP_NO_SEQ)
        drop = (t1['flag'] == 0).astype(np.uint8)  # 6 tabs or fewer: never printed
        drop[asked] = index.purge_flags(t1['seq'][asked], t1['c0'][asked], t1['c1'][asked])
        clock.lap('kernels')
        text = plan.render(drop)
        clock.lap('render')
        return text, None
    finally:
        if index is not None:
            index.close()
        plan.close()


def purge_overlaps(gff1, gff_to_purge, native='True'):
    """genome_tools.py:548-568: the lines of ``gff_to_purge`` that overlap no
    line of ``gff1`` on the same seqid.  Only lines with more than 6 tabs are
    read ('#' lines among them) and only they are printed; one whose seqid
    ``gff1`` lacks is printed without its integers being read.  A line (c0, c1) is
    dropped when an interval (p0, p1) of ``gff1`` has p0 < c0 < p1,
    p0 < c1 < p1 or c0 < p0 < c1, all strict and on the integers as parsed:
    touching, equal and reversed intervals do not count.  A printed line loses
    its last byte (its LF; the last byte of a final line without one) and gets
    an LF.

    On the device (engine.IntervalIndex: the first file's intervals sorted,
    a few binary searches per line) unless an integer does not parse, lies
    beyond the index's coordinate range, or there are 2^24 seqids: then, and
    with ``native=False``, the line loop below restates the reference, its
    ValueError after the lines printed so far included.  Nothing is written
    before the path is known.  ``purge_overlaps.last_path`` names the path the
    last call took."""
    clock = _Clock()
    first, second = _map_file(gff1), _map_file(gff_to_purge)
    clock.lap('open')
    if native == 'True':
        text, why = _purge_native(first, second, clock)
        if text is not None:
            purge_overlaps.last_path = ('purge_overlaps', 'native', None)
            _write_bytes(text)
            clock.lap('write')
            clock.emit()
            return
    else:
        why = "native != 'True'"
    purge_overlaps.last_path = ('purge_overlaps', 'host', why)
    out = []
    try:
        _purge_host(first, second, out)
    finally:
        _write_bytes(*out)
    clock.lap('write')
    clock.emit()


purge_overlaps.last_path = None


_PSL_PASS = (b'p', b'\n', b'm', b'-', b'\t', b' ')


def _besthits_host(data, order, out):
    """The reference's loop restated; what it prints is appended to ``out`` as
    it goes, so the pass-through lines before an error line are there."""
    best = {}  # key -> [score, line]; a dict keeps first-seen order
    for line in _lines_of(data):
        if line[:1] in _PSL_PASS:
            out.append(line[:-1] + b'\n')
            continue
        fields = line.split(b'\t')
        try:
            key = fields[9]
            score = _py2_int(fields[0]) - _py2_int(fields[1])
        except (IndexError, ValueError):  # the reference's bare except
            out.append(line + b'\n')
            return
        if key not in best or score > best[key][0]:
            best[key] = [score, line[:-1]]
    keys = list(best)
    if order == 'py2':
        from . import py2order
        text = py2order.dict_order([k.decode('latin-1') for k in keys])
        keys = [k.encode('latin-1') for k in text]
    for key in keys:
        out.append(best[key][1] + b'\n')


def _besthits_native(data, order, clock):
    """(besthits_from_psl's text as a uint8 array, None) from the device:
    engine.BestHits' pass-through lines in file order, then each key's best
    line, in first-seen order or in the order a Python 2 dict of the keys
    iterates (from the hashes the device computed).  (None, reason) when only
    the line loop is exact."""
    hits = engine.BestHits.parse(data)
    clock.lap('kernels')
    if isinstance(hits, tuple):
        return hits
    try:
        p_off, p_len = hits.pass_lines()
        g = hits.groups()
        off, length = g['off'], g['len']
        if order == 'py2':
            perm = engine.py2_order_of_hashes(g['hash'])
            off, length = off[perm], length[perm]
        clock.lap('order')
        text = engine.render_lines(data, np.concatenate([p_off, off]),
                                   np.concatenate([p_len, length]))
        clock.lap('render')
        return text, None
    finally:
        hits.close()


def besthits_from_psl(psl, order='py2', native='True'):
    """genome_tools.py:572-592: for every query name of a BLAT PSL file the
    line with the highest matches - misMatches.  Lines end at LF only.  A line
    whose first byte is one of ``p``, LF, ``m``, ``-``, TAB, space (the
    ``psLayout`` header, blank lines) is printed at once; every other line is
    split at its tabs: field 9 is the key -- with the LF, and a CR before it,
    when it is the last field -- and int(field 0) - int(field 1) the score.  A
    key's first line is kept and replaced only by a strictly greater score.  A
    line with fewer than 10 fields or an integer Python 2 rejects is printed
    whole (its LF and another) and ends the run: no winner is printed.
    Otherwise the winners follow, in the order a Python 2 dict of the keys
    iterates (``order='py2'``) or first seen (``order='insertion'``).  A
    printed line loses its last byte (its LF; the last byte of a final line
    without one) and gets an LF.

    On the device (engine.BestHits: a line index, one lane per line, the lines
    grouped by the key's hash with a sort, every group verified byte for byte,
    a segmented maximum) unless a data line is outside the native grammar --
    fewer than 10 fields, or field 0 or 1 not 1 to 10 digits alone with a value
    up to 2^31 - 1 --, two keys collide, or the text is too large for the
    device: then, and with ``native=False``, the line loop on the host restates
    the reference.  Nothing is written before the path is known.
    ``besthits_from_psl.last_path`` names the path the last call took."""
    if order not in ('py2', 'insertion'):
        raise ValueError("order must be 'py2' or 'insertion'")
    clock = _Clock()
    data = _map_file(psl)
    clock.lap('open')
    if native == 'True':
        text, why = _besthits_native(data, order, clock)
        if text is not None:
            besthits_from_psl.last_path = ('besthits_from_psl', 'native', None)
            _write_bytes(text)
            clock.lap('write')
            clock.emit()
            return
    else:
        why = "native != 'True'"
    besthits_from_psl.last_path = ('besthits_from_psl', 'host', why)
    out = []
    try:
        _besthits_host(data, order, out)
    finally:
        _write_bytes(*out)
    clock.lap('write')
    clock.emit()


besthits_from_psl.last_path = None



def _composition_host(fasta_alignment, order):
    """The reference's loops restated over genome.GenomeSequence; the text it
    prints once they are through."""
    seq_dict = genome.GenomeSequence(fasta_alignment)
    names = list(seq_dict)
    if order == 'py2':
        from . import py2order
        names = py2order.dict_order(names)
    position_list = [['a', 't', 'c', 'g']]
    for site in range(len(seq_dict[names[0]])):  # no record: IndexError
        count_dict = {'a': 0, 't': 0, 'c': 0, 'g': 0}
        allcounts = 0
        for name in names:
            cell = seq_dict[name][site].lower()  # a shorter record: IndexError
            if cell in count_dict:
                count_dict[cell] += 1
                allcounts += 1
        position_list.append([_py2_float_str(count_dict[n] * 1.0 / allcounts)  # ZeroDivisionError
                              for n in position_list[0]])
    return ''.join('\t'.join(position) + '\n' for position in position_list)


def _composition_native(fasta_alignment, order, clock):
    """(composition_by_site's text as a uint8 array, None) from the device: the
    FASTA packed natively, engine.SiteCounts over its records as rows,
    engine.render_composition on the host.  (None, reason) where the records
    the native reader sees are not the reference's dict.  Raises the
    reference's IndexError and ZeroDivisionError."""
    fa = genome.read_buffer(fasta_alignment)
    if len(fa) == 0:
        return None, 'no records'
    if bytes(fa[:1]) != b'>':
        return None, 'text before the first header'
    found = engine.fasta_contigs(fa)
    clock.lap('fasta_index')
    if found is None:
        return None, 'the native reader refuses the file'
    names, lengths = found
    if not names:
        return None, 'no records'
    if sum(lengths) > engine.PART_BASES:
        return None, 'more bases than one plane'
    first = names[0]
    if order == 'py2':
        from . import py2order
        first = py2order.dict_order(names)[0]
    n_sites = lengths[names.index(first)]
    # The reference divides at every site before it reaches the next one, so
    # with a record shorter than the first it raises at that record's end --
    # unless a site before it has no counted base.  The sites up to there are
    # counted to tell the two apart.
    shortest = min(lengths)
    clock.lap('order')
    dev = sites = None
    try:
        dev = engine.FastaGenome.load(fa, truncate_names=False)
        clock.lap('fasta_read')
        if dev is None:
            return None, 'the native reader refuses the file'
        sites = engine.SiteCounts(dev, n_sites=min(n_sites, shortest))
        counts = sites.counts()
        clock.lap('kernels')
        _composition_native.calls += 1
        if shortest < n_sites:
            if not counts.any(axis=1).all():
                raise ZeroDivisionError('float division by zero')
            raise IndexError('string index out of range')
        text = engine.render_composition(counts)
        clock.lap('render')
        return text, None
    finally:
        for obj in (sites, dev):
            if obj is not None:
                obj.close()


_composition_native.calls = 0  # device passes so far


def composition_by_site(fasta_alignment, order='py2', native='True'):
    """genome_tools.py:488-503: for every column of a FASTA alignment the
    share of a, t, c and g among the records that hold one of the four there,
    in either case; N, '-', IUPAC and every other byte count neither as a base
    nor in the denominator.  The header line ``a\\tt\\tc\\tg``, then one
    line per site of the four shares as Python 2 prints a float.  The number of
    sites is the length of the dict's first record: the first in the order a
    Python 2 dict of the names iterates (``order='py2'``) or the first in the
    file (``order='insertion'``).  Longer records are read up to there; a
    shorter one is an IndexError, a site without a counted base a
    ZeroDivisionError, no record an IndexError, and nothing is printed then:
    the reference prints after its loops.

    On the device (engine.SiteCounts: one pass across the records of the
    packed genome; engine.render_composition for the text) for a regular
    file that starts with a header, whose records the native reader takes,
    with at most one device plane of bases; the native reader folds a repeated
    name as the dict does (first position, last sequence).  Otherwise,
    and with ``native=False``, the loops on the host restate the reference
    over genome.GenomeSequence, a string that names no file read as the text
    itself included.  With a record shorter than the first, the device counts
    the sites before that record's end, to raise ZeroDivisionError where the
    reference meets an empty site first, IndexError otherwise.
    ``composition_by_site.last_path`` names the path the last call took."""
    if order not in ('py2', 'insertion'):
        raise ValueError("order must be 'py2' or 'insertion'")
    clock = _Clock()
    if native != 'True':
        why = "native != 'True'"
    elif not (isinstance(fasta_alignment, str) and os.path.isfile(fasta_alignment)):
        why = 'not a regular file'
    else:
        composition_by_site.last_path = ('composition_by_site', 'native', None)
        text, why = _composition_native(fasta_alignment, order, clock)
        if text is not None:
            _write_bytes(text)
            clock.lap('write')
            clock.emit()
            return
    composition_by_site.last_path = ('composition_by_site', 'host', why)
    _write(_composition_host(fasta_alignment, order))
    clock.lap('write')
    clock.emit()


composition_by_site.last_path = None


def heterozygosity_from_vcf(vcf, window='10000', loci=None, order='py2', native='True'):
    """magot_variants.heterozygosity_from_vcf from the command line: the
    windowed het rates of a VCF (magot_variants.py:16-139).  ``loci`` names a
    file with one locus per line (``seqid,start,stop`` or ``seqid,length``;
    empty lines are left out); without it the loci are the windows of the
    header's contig lines.  The function's three prints, then the string it
    returns, as Python 2's ``print`` writes it."""
    from . import magot_variants
    locus_list = None
    if loci is not None:
        text = genome.read_bytes(loci).decode('latin-1')
        locus_list = [ln for ln in text.replace('\r', '').split('\n') if ln]
    result = magot_variants.heterozygosity_from_vcf(vcf, locus_list, _literal(window), order=order,
                                                    native=native)
    heterozygosity_from_vcf.last_path = magot_variants.heterozygosity_from_vcf.last_path
    _write(str(result) + '\n')


heterozygosity_from_vcf.last_path = None


def _exclusion_names(exclude_list):
    """genome_tools.py:381-384 as bytes: the lines of the file ``exclude_list``
    names, every CR dropped (a file that ends in LF gives b'' too); when that
    raises anything at all, the text itself split at its commas."""
    try:
        with open(exclude_list, 'rb') as fh:
            return fh.read().replace(b'\r', b'').split(b'\n')
    except Exception:  # noqa: BLE001  (the reference's bare except)
        return exclude_list.encode('latin-1').split(b',')


def _exclude_host(fasta, names, first_word, order, out):
    """The reference's loop restated over genome.GenomeSequence; what it prints
    is appended to ``out`` as it goes, so the records before a key without a
    word are there when the IndexError leaves."""
    seqs = genome.GenomeSequence(fasta)
    keys = list(seqs)
    if order == 'py2':
        from . import py2order
        keys = py2order.dict_order(keys)
    listed = set(names)
    for key in keys:
        name = key.encode('latin-1')
        compared = name.split()[0] if first_word else name  # bytes.split: Python 2's blanks
        if compared not in listed:
            out.append(b'>' + name + b'\n' + seqs[key].encode('latin-1') + b'\n')


def _exclude_native(fasta, names, first_word, order, clock):
    """(exclude_from_fasta's text as a uint8 array, None) from the device:
    engine.FastaRecords' keys less the listed ones, in first-seen order or in
    the order a Python 2 dict of them iterates (from the hashes the device
    computed), each with its last sequence on one line.  (None, reason) when
    only the host loop is exact."""
    data = genome.read_buffer(fasta)
    clock.lap('open')
    recs = engine.FastaRecords.parse(data)
    clock.lap('kernels')
    if isinstance(recs, tuple):
        return recs
    try:
        keys = recs.keys()
        if first_word and keys['no_word'].any():
            return None, 'a key without a word'
        keep = recs.exclude(names, first_word=first_word)
        clock.lap('membership')
        last = keys['last_record']
        if order == 'py2':
            perm = engine.py2_order_of_hashes(keys['hash'])
            last, keep = last[perm], keep[perm]
        clock.lap('order')
        text = recs.render(last[keep], 'fasta')
        clock.lap('render')
        return text, None
    finally:
        recs.close()


def exclude_from_fasta(fasta, exclude_list, just_firstword='False', order='py2', native='True'):
    """genome_tools.py:377-391: a FASTA file without the records named in
    ``exclude_list`` -- a file of names, one per line, or, when no such file
    opens, the names themselves between commas.  The file is read as
    genome.GenomeSequence reads it: a record needs a sequence, a repeated name
    keeps its first place and its last sequence, text before the first header
    goes under the name ''.  With ``just_firstword='True'`` a record's first
    word is compared, not its name; a name without a word is an IndexError
    after the records before it.  Every record left is printed as ``>name``
    and its sequence on one line, in the order a Python 2 dict of the names
    iterates (``order='py2'``) or first seen (``order='insertion'``).

    On the device (engine.FastaRecords: the records indexed at a cost that
    does not depend on a line's length, grouped by name with a sort and
    verified, the list looked up by hash and compared byte for byte, the text
    reflowed by a grouped copy) for a regular file the device does not decline
    -- text before the first header, a CR in mid-line, a name above the lane's
    bound, two names in one hash bucket, a text too large -- and, with
    ``just_firstword='True'``, no key without a word.  Otherwise, and with
    ``native=False``, the loop on the host restates the reference, a string
    that names no file read as the text itself included.  Nothing is written
    before the path is known.  ``exclude_from_fasta.last_path`` names the path
    the last call took."""
    if order not in ('py2', 'insertion'):
        raise ValueError("order must be 'py2' or 'insertion'")
    clock = _Clock()
    first_word = just_firstword == 'True'
    names = _exclusion_names(exclude_list)
    clock.lap('list')
    if native != 'True':
        why = "native != 'True'"
    elif not (isinstance(fasta, str) and os.path.isfile(fasta)):
        why = 'not a regular file'
    else:
        text, why = _exclude_native(fasta, names, first_word, order, clock)
        if text is not None:
            exclude_from_fasta.last_path = ('exclude_from_fasta', 'native', None)
            _write_bytes(text)
            clock.lap('write')
            clock.emit()
            return
    exclude_from_fasta.last_path = ('exclude_from_fasta', 'host', why)
    out = []
    try:
        _exclude_host(fasta, names, first_word, order, out)
    finally:
        _write_bytes(*out)
    clock.lap('write')
    clock.emit()


exclude_from_fasta.last_path = None


def _fasta2tab_native(fasta_file, clock):
    """(fasta2tab's text as a uint8 array, None) from the device: every header
    of engine.FastaRecords in file order in the 'tab' style.  (None, reason)
    when only the host loop is exact.  Raises the reference's IndexError."""
    data = genome.read_buffer(fasta_file)
    clock.lap('open')
    if len(data) and bytes(data[:1]) != b'>':
        raise IndexError('list index out of range')  # newlines[-1] of an empty list
    recs = engine.FastaRecords.parse(data)
    clock.lap('kernels')
    if isinstance(recs, tuple):
        return recs
    try:
        text = recs.render(np.arange(recs.n_records, dtype=np.uint32), 'tab')
        clock.lap('render')
        return text, None
    finally:
        recs.close()


def fasta2tab(fasta_file, native='True'):
    """genome_tools.py:349-350 over magot_smallfuncs.py:21-29: every record of
    a FASTA file as ``name TAB sequence`` on one line, in file order; records
    without a sequence and repeated names all stay.  A line that is not a
    header before the first header is an IndexError, and nothing is printed.

    On the device (engine.FastaRecords and its reflow) for a regular file the
    device does not decline; otherwise, and with ``native=False``,
    genome.fasta2tab on the host.  ``fasta2tab.last_path`` names the path the
    last call took."""
    clock = _Clock()
    if native != 'True':
        why = "native != 'True'"
    elif not (isinstance(fasta_file, str) and os.path.isfile(fasta_file)):
        why = 'not a regular file'
    else:
        fasta2tab.last_path = ('fasta2tab', 'native', None)
        text, why = _fasta2tab_native(fasta_file, clock)
        if text is not None:
            _write_bytes(text)
            clock.lap('write')
            clock.emit()
            return
    fasta2tab.last_path = ('fasta2tab', 'host', why)
    _write(genome.fasta2tab(fasta_file) + '\n')
    clock.lap('write')
    clock.emit()


fasta2tab.last_path = None


def _tabcut_native(path, program, clock):
    """(the cut text as a uint8 array, None) from the device: engine.TabCut
    under ``program``.  (None, reason) where the device declines.  Raises the
    reference's IndexError for a short line the program reports."""
    data = genome.read_buffer(path)
    clock.lap('open')
    cut = engine.TabCut.parse(data, **program)
    clock.lap('kernels')
    if isinstance(cut, tuple):
        return cut
    try:
        if cut.short_line is not None:
            raise IndexError('list index out of range')  # fields[1] of a line without a TAB
        text = cut.render()
        clock.lap('render')
        return text, None
    finally:
        cut.close()


def tab2fasta(tab_file, native='True'):
    """genome_tools.py:345-346 over magot_smallfuncs.py:12-18: every line of a
    table as ``>`` its first field, LF, its second field, LF, in file order;
    further fields are dropped, and the LF and every CR of a line go before it
    is split.  A line without a TAB, an empty one included, is an IndexError,
    and nothing is printed.  An empty table prints one LF.

    On the device (engine.TabCut: the fields cut by their TAB offsets at a cost
    that does not depend on a line's length, the text written by a grouped copy)
    for a regular file the device does not decline -- a CR that is neither
    before an LF nor the file's last byte, a text too large; otherwise, and with
    ``native=False``, genome.tab2fasta on the host, a string that names no file
    read as the text itself included.  ``tab2fasta.last_path`` names the path
    the last call took."""
    clock = _Clock()
    if native != 'True':
        why = "native != 'True'"
    elif not (isinstance(tab_file, str) and os.path.isfile(tab_file)):
        why = 'not a regular file'
    else:
        tab2fasta.last_path = ('tab2fasta', 'native', None)
        text, why = _tabcut_native(tab_file, engine.TabCut.TAB2FASTA, clock)
        if text is not None:
            _write_bytes(text if len(text) else b'\n')  # `print ''`
            clock.lap('write')
            clock.emit()
            return
    tab2fasta.last_path = ('tab2fasta', 'host', why)
    _write(genome.tab2fasta(tab_file) + '\n')
    clock.lap('write')
    clock.emit()


tab2fasta.last_path = None


def _hints_host(data):
    """The reference's loop restated over bytes: every line with more than five
    TABs as its fields 0, 1, 3, 4 and 5 among the hint's constants."""
    out = []
    for line in data.split(b'\n'):
        if line.count(b'\t') > 5:  # the LF holds no TAB, and field 5 is never the last
            f = line.split(b'\t')
            out.append(b'\t'.join([f[0], f[1], b'nonexonpart', f[3], f[4], f[5], b'.', b'.',
                                   b'pri=2;src=RM']) + b'\n')
    return out


def repeatmasker2augustushints(repeatmasker_gff, native='True'):
    """genome_tools.py:449-454: a RepeatMasker GFF as AUGUSTUS hints.  Every
    line with more than five TABs prints its columns 1, 2, 4, 5 and 6 as
    ``c1 c2 nonexonpart c4 c5 c6 . . pri=2;src=RM``; every other line prints
    nothing, and ``#`` lines are lines like any other.  Nothing is stripped: a
    CR inside those columns is copied.  A path that does not open is an
    OSError.

    On the device (engine.TabCut) for a regular file the device does not
    decline; otherwise, and with ``native=False``, the loop on the host
    restates the reference.  ``repeatmasker2augustushints.last_path`` names the
    path the last call took."""
    clock = _Clock()
    with open(repeatmasker_gff, 'rb'):  # the reference's plain open
        pass
    if native != 'True':
        why = "native != 'True'"
    elif not (isinstance(repeatmasker_gff, str) and os.path.isfile(repeatmasker_gff)):
        why = 'not a regular file'
    else:
        text, why = _tabcut_native(repeatmasker_gff, engine.TabCut.HINTS, clock)
        if text is not None:
            repeatmasker2augustushints.last_path = ('repeatmasker2augustushints', 'native', None)
            _write_bytes(text)
            clock.lap('write')
            clock.emit()
            return
    repeatmasker2augustushints.last_path = ('repeatmasker2augustushints', 'host', why)
    with open(repeatmasker_gff, 'rb') as fh:
        _write_bytes(*_hints_host(fh.read()))
    clock.lap('write')
    clock.emit()


repeatmasker2augustushints.last_path = None


def _replace_table(table):
    """genome_tools.py:436-440 as bytes: (name, f1) of every line of the table
    in file order.  Lines end at LF only; f1 of a two-field line keeps its LF.
    A line without a TAB is the reference's IndexError."""
    rows = []
    for line in table.split(b'\n'):
        rows.append(line + b'\n')
    if rows[-1] == b'\n':  # what is behind the last LF: nothing
        rows.pop()
    else:
        rows[-1] = rows[-1][:-1]  # a last line without LF
    out = []
    for line in rows:
        fields = line.split(b'\t')
        if len(fields) < 2:
            raise IndexError('list index out of range')
        out.append((fields[0], fields[1]))
    return out


def _replace_dict(rows, name_end, order):
    """(names, values) of the dict the reference fills, in the order it is
    iterated (its keys are name + name_end): a repeated name keeps its first
    place and takes its last value."""
    table = {}
    for name, f1 in rows:
        table[name] = f1
    names = list(table)
    if order == 'py2':
        from . import py2order
        keys = py2order.dict_order([(n + name_end).decode('latin-1') for n in names])
        names = [k.encode('latin-1')[:len(k) - len(name_end)] for k in keys]
    return names, [table[n] for n in names]


def _replace_host(text, keys, values):
    """The reference's loop restated over bytes: for each line every key in
    dict order, each seeing the result of the keys before it; the line less its
    last byte, and an LF."""
    out = []
    lines = text.split(b'\n')
    last = lines.pop()
    lines = [line + b'\n' for line in lines] + ([last] if last else [])
    pairs = list(zip(keys, values))
    for line in lines:
        for word, new in pairs:
            if word in line:
                line = line.replace(word, new)
        out.append(line[:-1] + b'\n')
    return out


def _replace_chains(names, values):
    """Whether a key's value can feed a later key (names and values in rank
    order): some name_j, j after i, is a suffix of f1_i, or f1_i is a proper
    suffix of name_j.  Sets probed with every suffix: table bytes x longest
    name probes, never all pairs."""
    rank_of = {n: r for r, n in enumerate(names)}
    sizes = sorted({len(n) for n in names})  # only a suffix as long as a name can be one
    first_with = {}  # value -> the lowest rank that has it; only values shorter than a name
    for r, v in enumerate(values):
        if v.endswith(b'\n'):  # no name holds an LF: neither relation can hold
            continue
        if not v:  # a proper suffix of every name
            if r != len(names) - 1:
                return True
            continue
        if len(v) < sizes[-1]:
            first_with.setdefault(v, r)
        for k in sizes:
            if k > len(v):
                break
            if rank_of.get(v[len(v) - k:], -1) > r:
                return True
    if first_with:
        for r, n in enumerate(names):
            for k in range(1, len(n)):
                if first_with.get(n[len(n) - k:], r) < r:
                    return True
    return False


def _replace_decline(rows, name_end, order):
    """None when the device path prints what the reference prints, else the
    reason it is not taken; with None also the table for engine.NameReplacer:
    (names first seen, their last values, their ranks)."""
    if len(name_end) != 1 or name_end == b'\n':
        return 'name_end', None
    table = {}
    for name, f1 in rows:
        table[name] = f1
    names, values = list(table), list(table.values())
    if any(not n for n in names):
        return 'empty_name', None
    if max([len(n) for n in names] or [0]) > engine.NameReplacer.params()['max_name']:
        return 'long_name', None
    if any(name_end in n for n in names):
        return 'delimiter_in_name', None
    if any(name_end in v for v in values):
        return 'delimiter_in_value', None
    rank = np.arange(len(names), dtype=np.uint32)
    if order == 'py2' and names:
        perm = engine.py2_order_of_hashes(engine.py2_string_hashes([n + name_end for n in names]))
        rank[perm.astype(np.int64)] = np.arange(len(names), dtype=np.uint32)
    by_rank = np.argsort(rank, kind='stable')
    if _replace_chains([names[i] for i in by_rank], [values[i] for i in by_rank]):
        return 'chain', None
    return None, (names, values, rank)


def replace_names(text_file, replace_table, name_end=' ', order='py2', native='True'):
    """genome_tools.py:431-446: the words of a text renamed from a table.  Every
    line of ``replace_table`` is ``name TAB value``; the value of a two-field
    line keeps its LF (and a CR before it), a third field or a trailing TAB ends
    it before.  A line without a TAB is an IndexError before anything is
    printed.  A repeated name keeps its first place and takes its last value.
    For every line of ``text_file``, for every key ``name + name_end`` in the
    order a Python 2 dict of the keys iterates (``order='py2'``) or first seen
    (``order='insertion'``), all occurrences of the key become ``value +
    name_end``, each key seeing the result of the keys before it; the line is
    printed without its last byte (its LF; the last byte of a final line
    without one).  Lines end at LF only.

    On the device (engine.NameReplacer) for two regular files when ``name_end``
    is one byte other than LF, no name is empty, longer than the kernel's bound
    or holds ``name_end``, no value holds it, and no key's value feeds a later
    key (some later name a suffix of the value, or the value a proper suffix of
    a later name): then a field between two delimiters is rewritten at most
    once, by the first key in dict order whose name is a suffix of it.
    Otherwise, where the device declines and with ``native=False``, the loop on
    the host restates the reference.  Nothing is written before the path is
    known.  ``replace_names.last_path`` names the path the last call took."""
    if order not in ('py2', 'insertion'):
        raise ValueError("order must be 'py2' or 'insertion'")
    clock = _Clock()
    name_end = name_end.encode('latin-1')
    with open(text_file, 'rb'):  # the reference opens the text first
        pass
    with open(replace_table, 'rb') as fh:
        rows = _replace_table(fh.read())
    clock.lap('table')
    text = None
    if native != 'True':
        why = "native != 'True'"
    elif not all(isinstance(p, str) and os.path.isfile(p) for p in (text_file, replace_table)):
        why = 'not a regular file'
    else:
        why, table = _replace_decline(rows, name_end, order)
        clock.lap('decision')
        if why is None:
            data = genome.read_buffer(text_file)
            clock.lap('open')
            names, values, rank = table
            rep = engine.NameReplacer.parse(data, names, values, name_end, rank)
            clock.lap('kernels')
            if isinstance(rep, tuple):
                why = rep[1]
            else:
                try:
                    text = rep.render()
                finally:
                    rep.close()
                clock.lap('render')
    if text is not None:
        replace_names.last_path = ('replace_names', 'native', None)
        _write_bytes(text)
    else:
        replace_names.last_path = ('replace_names', 'host', why)
        with open(text_file, 'rb') as fh:
            data = fh.read()
        names, values = _replace_dict(rows, name_end, order)
        _write_bytes(*_replace_host(data, [n + name_end for n in names],
                                    [v + name_end for v in values]))
    clock.lap('write')
    clock.emit()


replace_names.last_path = None


def convert_gff(gff, input_format, output_format, order='py2', native='True'):
    """genome_tools.py:527-545: an annotation read in one format and written in
    another.  ``input_format``: ``gff3`` (also the name under which a GTF with
    ``gene_id``/``transcript_id`` is read) or a preset of ``read_gff``;
    ``output_format``: ``gff3``, ``gtf`` or ``exon_added_gff3``.

    On the device (engine.GffWriter) when ``input_format`` names no preset and
    the host planner can lower the annotation to output rows; otherwise, where
    the planner or the device declines and with ``native=False``, ``write_gff``
    on the host restates the reference, its exceptions included.  Nothing is
    written before the path is known.  ``convert_gff.last_path`` names the path
    the last call took."""
    if order not in ('py2', 'insertion'):
        raise ValueError("order must be 'py2' or 'insertion'")
    if input_format == 'gff3':
        presets = None
    else:
        presets = input_format
    if output_format == 'gff3':
        gff_format = "simple gff3"
    elif output_format == 'gtf':
        gff_format = 'gtf'
    elif output_format == "exon_added_gff3":
        gff_format = "exon added gff3"
    else:
        _write("currently only writes 'gff3' and 'gtf' format\n")
        return None
    text = None
    if native != 'True':
        why = "native != 'True'"
    elif presets in genome._PRESETS:
        why = 'preset'
    elif not (isinstance(gff, str) and os.path.isfile(gff)):
        why = 'not a regular file'
    else:
        text, why = _convert_gff_native(gff, gff_format, order)
    if text is not None:
        convert_gff.last_path = ('convert_gff', 'native', None)
        _write_bytes(text, b'\n')
    else:
        convert_gff.last_path = ('convert_gff', 'host', why)
        annotations = genome.read_gff(gff, presets=presets)
        _write(genome.write_gff(annotations, gff_format, order) + '\n')


convert_gff.last_path = None


def _convert_gff_native(gff, gff_format, order):
    """(text, None) from the planner's rows rendered on the device, or
    (None, why) where the planner or the device declines."""
    data = genome.read_buffer(gff)
    read = engine.GffRead.read(data, for_write=True)
    if read is None:
        return None, 'read_gff takes a diagnostic path'
    try:
        plan = read.lower_write(gff_format, order)
        if plan is None:
            return None, 'write_gff takes a diagnostic path'
        if not len(plan.rows):
            return b'', None  # '\n'.join of no line
        writer = engine.GffWriter.parse(data, plan.blob, plan.rows)
        if isinstance(writer, tuple):
            return None, writer[1]
        try:
            out = writer.render()
        finally:
            writer.close()
        return out[:-1], None  # write_gff joins the lines: the last has no LF
    finally:
        read.close()


TOOLS = {'gff2fasta': gff2fasta, 'cds2pep': cds2pep, 'at_content_from_fasta': at_content_from_fasta,
         'fqstats': fqstats, 'purge_overlaps': purge_overlaps, 'besthits_from_psl': besthits_from_psl,
         'extract_upstream_downstream': extract_upstream_downstream,
         'coords2fasta': coords2fasta,
         'blast_csv2fasta': blast_csv2fasta, 'exonerate2fasta': exonerate2fasta,
         'get_seq_from_fasta': get_seq_from_fasta, 'dna2orfs': dna2orfs,
         'mask_from_gff': mask_from_gff, 'depth_from_gff': depth_from_gff,
         'composition_by_site': composition_by_site,
         'heterozygosity_from_vcf': heterozygosity_from_vcf,
         'exclude_from_fasta': exclude_from_fasta, 'fasta2tab': fasta2tab,
         'replace_names': replace_names, 'convert_gff': convert_gff, 'tab2fasta': tab2fasta,
         'repeatmasker2augustushints': repeatmasker2augustushints,
         'get_CDS_peptides': get_CDS_peptides}


def parse_argv(argv):
    """['tool', 'pos', 'k=v', ...] -> (tool, positional, keywords) as the
    reference's main() assembles them (genome_tools.py:35-44: only the text
    between the first and second '=' is the value)."""
    name = argv[0]
    args, kw = [], {}
    for a in argv[1:]:
        if '=' in a:
            parts = a.split('=')
            kw[parts[0]] = parts[1]
        else:
            args.append(a)
    return name, args, kw


def main(argv=None):
    argv = sys.argv[1:] if argv is None else argv
    if not argv or argv[0] in ('-h', '-help', '--help', 'help'):
        sys.stdout.write(__doc__)
        return 0
    name, args, kw = parse_argv(argv)
    if name not in TOOLS:
        sys.stderr.write('unknown tool %r (extraction path tools: %s)\n'
                         % (name, ', '.join(sorted(TOOLS))))
        return 2
    TOOLS[name](*args, **kw)
    return 0


if __name__ == '__main__':
    sys.exit(main())
