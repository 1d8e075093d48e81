"""Device-level objects over the C ABI: packed genome, extraction plan, and the
raw-sequence batch ops.  Everything here runs on the GPU through libmagot.so;
there is no host compute path."""

import ctypes
import os

import numpy as np

from . import _lib
from ._lib import (EXON_DTYPE, TX_DTYPE, OUT_NUC, OUT_PEP, OUT_GENOME_ORDER, MagotError, check,
                   ptr)


def _as_bytes(s):
    if isinstance(s, (bytes, bytearray, memoryview)):
        return bytes(s)
    return s.encode('latin-1')


def _text_view(s):
    """A uint8 view of text for the native parsers without copying: bytes,
    bytearray, mmap (genome.read_buffer) or numpy; str is encoded."""
    if isinstance(s, str):
        s = s.encode('latin-1')
    if isinstance(s, np.ndarray):
        return np.ascontiguousarray(s).view(np.uint8).reshape(-1)
    return np.frombuffer(s, dtype=np.uint8)


def _text_ptr(view):
    return view.ctypes.data if len(view) else None


class DeviceGenome(object):
    """A GenomeSequence packed into HBM (magot_genome_load).

    ``contigs`` is a list of (name, sequence) pairs; sequences are ``str``
    (latin-1, one char per byte), ``bytes`` or uint8 numpy arrays.
    """

    def __init__(self, contigs, ctx=None, pack='device'):
        """``pack``: 'device' (default: raw bytes streamed to HBM once, packed
        by kernels) or 'host' (pack.cpp, then the plane uploaded)."""
        if pack not in ('device', 'host'):
            raise ValueError(pack)
        self.ctx = ctx or _lib.default_context()
        names = []
        bufs = []
        for name, seq in contigs:
            names.append(name)
            if isinstance(seq, np.ndarray):  # a uint8 view (no copy)
                bufs.append(np.ascontiguousarray(seq).view(np.uint8).reshape(-1))
            else:
                bufs.append(np.frombuffer(_as_bytes(seq), dtype=np.uint8))
        n = len(bufs)
        self.names = names
        self.index = {nm: i for i, nm in enumerate(names)}
        self.lengths = np.array([len(b) for b in bufs], dtype=np.uint64)
        ptrs = (ctypes.POINTER(ctypes.c_uint8) * max(n, 1))()
        for i, b in enumerate(bufs):
            if len(b):
                ptrs[i] = b.ctypes.data_as(ctypes.POINTER(ctypes.c_uint8))
        lens = np.ascontiguousarray(self.lengths)
        h = ctypes.c_void_p()
        L = _lib.lib()
        flags = _lib.PACK_HOST if pack == 'host' else 0
        check(L.magot_genome_load_ex(self.ctx.handle, ptrs, lens.ctypes.data_as(_lib._u64p), n,
                                     flags, ctypes.byref(h)), 'magot_genome_load')
        self.handle = h
        self._keepalive = None
        self._stats()

    def _check_contigs(self):
        """The caller's contig lengths against the genome's own table (a
        replica built from a meta blob of another genome is refused)."""
        n = ctypes.c_uint32()
        nl = ctypes.c_uint64()
        L = _lib.lib()
        check(L.magot_genome_contigs(self.handle, ctypes.byref(n), None, None, 0,
                                     ctypes.byref(nl)), 'magot_genome_contigs')
        lens = np.zeros(max(n.value, 1), dtype=np.uint64)
        check(L.magot_genome_contigs(self.handle, ctypes.byref(n), ptr(lens), None, 0,
                                     ctypes.byref(nl)), 'magot_genome_contigs')
        if n.value != len(self.names) or not np.array_equal(lens[:n.value], self.lengths):
            self.close()
            raise MagotError('genome replica: %d contigs in the meta blob, %d names / lengths '
                             'given, or their lengths differ' % (n.value, len(self.names)))

    def _stats(self):
        tb, nr, db = ctypes.c_uint64(), ctypes.c_uint64(), ctypes.c_uint64()
        check(_lib.lib().magot_genome_stats(self.handle, ctypes.byref(tb), ctypes.byref(nr),
                                            ctypes.byref(db)), 'magot_genome_stats')
        self.total_bases = tb.value
        self.n_exception_runs = nr.value
        self.device_bytes = db.value

    # -- replication (magot_genome_export / copy_arena / attach) -------------
    def export(self):
        """(meta bytes, arena size in bytes) of the packed genome."""
        L = _lib.lib()
        n, ab = ctypes.c_uint64(), ctypes.c_uint64()
        check(L.magot_genome_export(self.handle, None, 0, ctypes.byref(n), ctypes.byref(ab)),
              'magot_genome_export')
        meta = np.empty(n.value, dtype=np.uint8)
        check(L.magot_genome_export(self.handle, ptr(meta), n.value, ctypes.byref(n),
                                    ctypes.byref(ab)), 'magot_genome_export')
        return meta.tobytes(), ab.value

    def wire_ranges(self):
        """[(offset, length)] of the arena a replica must receive (the forward
        plane, then runs + directory); the mirror is rebuilt on attach."""
        off = np.zeros(2, dtype=np.uint64)
        ln = np.zeros(2, dtype=np.uint64)
        n = ctypes.c_uint32()
        check(_lib.lib().magot_genome_wire_ranges(self.handle, off.ctypes.data_as(_lib._u64p),
                                                  ln.ctypes.data_as(_lib._u64p), ctypes.byref(n)),
              'magot_genome_wire_ranges')
        return [(int(off[k]), int(ln[k])) for k in range(n.value)]

    def wire_size(self):
        """Bytes of the compact replica image (magot_genome_wire_export)."""
        n = ctypes.c_uint64()
        check(_lib.lib().magot_genome_wire_export(self.handle, None, 0, ctypes.byref(n)),
              'magot_genome_wire_export')
        return n.value

    def wire_export(self, dst_dev_ptr, cap):
        """Write the compact replica image (2-bit codes, soft-mask runs,
        exception runs) into caller device memory of ``cap`` bytes; returns
        its size."""
        n = ctypes.c_uint64()
        check(_lib.lib().magot_genome_wire_export(self.handle, ctypes.c_void_p(dst_dev_ptr),
                                                  int(cap), ctypes.byref(n)),
              'magot_genome_wire_export')
        return n.value

    @classmethod
    def from_wire(cls, meta, wire_dev_ptr, wire_bytes, names, lengths, ctx=None):
        """A genome rebuilt on this device from a replica image in device
        memory (magot_genome_wire_import); it owns its arena, and the image
        can be freed afterwards."""
        self = cls.__new__(cls)
        self.ctx = ctx or _lib.default_context()
        self.names = list(names)
        self.index = {nm: i for i, nm in enumerate(self.names)}
        self.lengths = np.asarray(lengths, dtype=np.uint64)
        self._keepalive = None
        m = np.frombuffer(meta, dtype=np.uint8)
        h = ctypes.c_void_p()
        check(_lib.lib().magot_genome_wire_import(self.ctx.handle, ptr(m), len(m),
                                                  ctypes.c_void_p(wire_dev_ptr), int(wire_bytes),
                                                  ctypes.byref(h)), 'magot_genome_wire_import')
        self.handle = h
        self._check_contigs()
        self._stats()
        return self

    def copy_arena(self, dst_dev_ptr):
        """D2D copy of the packed arena to caller device memory (an address)."""
        check(_lib.lib().magot_genome_copy_arena(self.handle, ctypes.c_void_p(dst_dev_ptr)),
              'magot_genome_copy_arena')

    @classmethod
    def attach(cls, meta, arena_dev_ptr, names, lengths, ctx=None, keepalive=None, wire=False):
        """A genome over caller device memory that holds a broadcast arena.
        ``keepalive`` (e.g. the tensor owning the memory) lives as long as this.
        ``wire=True``: the memory holds only the wire ranges; the mirror plane
        is rebuilt on this device (magot_genome_attach_wire)."""
        self = cls.__new__(cls)
        self.ctx = ctx or _lib.default_context()
        self.names = list(names)
        self.index = {nm: i for i, nm in enumerate(self.names)}
        self.lengths = np.asarray(lengths, dtype=np.uint64)
        self._keepalive = keepalive
        m = np.frombuffer(meta, dtype=np.uint8)
        h = ctypes.c_void_p()
        fn = _lib.lib().magot_genome_attach_wire if wire else _lib.lib().magot_genome_attach
        check(fn(self.ctx.handle, ptr(m), len(m), ctypes.c_void_p(arena_dev_ptr), ctypes.byref(h)),
              'magot_genome_attach')
        self.handle = h
        self._check_contigs()
        self._stats()
        return self

    def close(self):
        if getattr(self, 'handle', None):
            _lib.lib().magot_genome_destroy(self.handle)
            self.handle = None
        self._keepalive = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


# One device plane addresses < 4 Gbases (32-bit window offsets, extract.hip);
# a larger genome is packed as several planes (PartitionedGenome).  The C side
# refuses a plane whose packed span (kOrigin=64 pad bases + bases + 256) reaches
# 0xFFFFFFF0 (magot_genome_load), so the part size is clamped below that.
PLANE_LIMIT = 0xFFFFFFF0 - 64 - 256 - 1
PART_BASES = min(int(os.environ.get('MAGOT_GENOME_PART_BASES', '3500000000')), PLANE_LIMIT)


def plan_parts(lengths, limit=None):
    """Contigs (in order) -> part index per contig: consecutive contigs share
    a part while its bases stay <= limit.  A contig above the limit cannot be
    packed (MagotError)."""
    limit = PART_BASES if limit is None else limit
    part = np.zeros(len(lengths), dtype=np.int64)
    k, acc = 0, 0
    for i, n in enumerate(int(x) for x in lengths):
        if n > limit:
            raise MagotError('contig %d has %d bases: above the %d-base device plane' %
                             (i, n, limit))
        if acc and acc + n > limit:
            k, acc = k + 1, 0
        part[i] = k
        acc += n
    return part


class PartitionedGenome(object):
    """A genome above one device plane: contigs cut into parts (plan_parts),
    each packed into its own HBM arena.  Extraction over it runs one plan per
    part (extract_records)."""

    def __init__(self, contigs, ctx=None, limit=None):
        contigs = list(contigs)
        self.ctx = ctx or _lib.default_context()
        self.names = [n for n, _ in contigs]
        self.index = {nm: i for i, nm in enumerate(self.names)}
        self.lengths = np.array([len(s) for _, s in contigs], dtype=np.uint64)
        self.part_of = plan_parts(self.lengths, limit)
        n_parts = int(self.part_of.max()) + 1 if len(contigs) else 0
        self.local = np.zeros(len(contigs), dtype=np.int64)
        self.parts = []
        for k in range(n_parts):
            idx = np.nonzero(self.part_of == k)[0]
            self.local[idx] = np.arange(len(idx))
            self.parts.append(DeviceGenome([contigs[i] for i in idx], ctx=self.ctx))
        self.total_bases = int(self.lengths.sum())

    def close(self):
        for g in self.parts:
            g.close()
        self.parts = []


def device_genome(contigs, ctx=None):
    """DeviceGenome, or PartitionedGenome above PART_BASES bases."""
    contigs = list(contigs)
    if sum(len(s) for _, s in contigs) > PART_BASES:
        return PartitionedGenome(contigs, ctx=ctx)
    return DeviceGenome(contigs, ctx=ctx)


def extract_records(genome, exons, txs, outputs=OUT_NUC | OUT_PEP):
    """ExtractionPlan(genome, exons, txs, outputs).run() over either genome
    kind.  On a PartitionedGenome: one plan (one launch) per part; a record
    whose intervals lie in two parts is gathered as one-interval pieces in
    their parts, joined, and translated in one translate_batch launch."""
    if not isinstance(genome, PartitionedGenome):
        plan = ExtractionPlan(genome, exons, txs, outputs)
        try:
            return plan.run()
        finally:
            plan.close()
    exons = np.ascontiguousarray(exons, dtype=EXON_DTYPE)
    txs = np.ascontiguousarray(txs, dtype=TX_DTYPE)
    T = len(txs)
    begin = txs['exon_begin'].astype(np.int64)
    count = txs['n_exons'].astype(np.int64)
    ex_part = genome.part_of[exons['contig'].astype(np.int64)] if len(exons) else \
        np.zeros(0, np.int64)
    rec_part = np.zeros(T, dtype=np.int64)
    cross = np.zeros(T, dtype=bool)
    for t in np.nonzero(count > 0)[0]:
        ps = ex_part[begin[t]:begin[t] + count[t]]
        rec_part[t] = ps[0]
        cross[t] = bool((ps != ps[0]).any())
    rec_len = np.zeros(T, dtype=np.int64)
    if len(exons):
        cs = np.concatenate([[0], np.cumsum(exons['len'].astype(np.int64))])
        rec_len = cs[begin + count] - cs[begin]
    noff = np.zeros(T + 1, dtype=np.uint64)
    np.cumsum(rec_len, out=noff[1:])
    want_pep = bool(outputs & OUT_PEP)
    pep_len = rec_len // 3
    poff = np.zeros(T + 1, dtype=np.uint64)
    np.cumsum(pep_len, out=poff[1:])
    nuc = np.empty(int(noff[-1]), dtype=np.uint8) if outputs & OUT_NUC or cross.any() else None
    pep = np.empty(int(poff[-1]), dtype=np.uint8) if want_pep else None
    for k, part in enumerate(genome.parts):
        whole = np.nonzero((rec_part == k) & ~cross)[0]
        pieces = [e for t in np.nonzero(cross)[0]
                  for e in range(begin[t], begin[t] + count[t]) if ex_part[e] == k]
        if len(whole) == 0 and not pieces:
            continue
        sub_ex = [exons[begin[t]:begin[t] + count[t]] for t in whole] + \
            [exons[e:e + 1] for e in pieces]
        sub_ex = np.concatenate(sub_ex) if sub_ex else np.zeros(0, EXON_DTYPE)
        sub_ex['contig'] = genome.local[sub_ex['contig'].astype(np.int64)]
        cnt = np.concatenate([count[whole], np.ones(len(pieces), np.int64)])
        sub_tx = np.zeros(len(cnt), dtype=TX_DTYPE)
        sub_tx['n_exons'] = cnt
        sub_tx['exon_begin'] = np.cumsum(cnt) - cnt
        sub_out = outputs | (OUT_NUC if pieces else 0)
        n_k, no_k, p_k, po_k = extract_records(part, sub_ex, sub_tx, sub_out)
        for i, t in enumerate(whole):
            if nuc is not None and n_k is not None:
                nuc[int(noff[t]):int(noff[t + 1])] = n_k[int(no_k[i]):int(no_k[i + 1])]
            if want_pep:
                pep[int(poff[t]):int(poff[t + 1])] = p_k[int(po_k[i]):int(po_k[i + 1])]
        piece_bytes = {}
        for j, e in enumerate(pieces):
            i = len(whole) + j
            piece_bytes[e] = n_k[int(no_k[i]):int(no_k[i + 1])]
        for t in np.nonzero(cross)[0]:
            o = int(noff[t])
            for e in range(begin[t], begin[t] + count[t]):
                ln = int(exons['len'][e])
                if e in piece_bytes:
                    nuc[o:o + ln] = piece_bytes[e]
                o += ln
    if want_pep and cross.any():
        ids = np.nonzero(cross)[0]
        seqs = [nuc[int(noff[t]):int(noff[t + 1])].tobytes().decode('latin-1') for t in ids]
        peps = translate_batch(seqs, [0] * len(seqs), ['+'] * len(seqs))
        for t, pstr in zip(ids, peps):
            pep[int(poff[t]):int(poff[t + 1])] = np.frombuffer(
                (pstr or '').encode('latin-1'), dtype=np.uint8)
    if not outputs & OUT_NUC:
        nuc = None
    return nuc, noff, pep, poff


def _fasta_index(L, tp, size, truncate_names):
    """(count, lengths, NUL-separated name bytes) of a FASTA text, or None."""
    n = ctypes.c_uint32()
    nl = ctypes.c_uint64()
    rc = L.magot_fasta_read(tp, size, int(bool(truncate_names)), ctypes.byref(n), None,
                            None, 0, ctypes.byref(nl), None, 0)
    if rc == _lib.ERR_UNSUPPORTED:
        return None
    check(rc, 'magot_fasta_read')
    lens = np.zeros(max(n.value, 1), dtype=np.uint64)
    names = np.zeros(max(nl.value, 1), dtype=np.uint8)
    check(L.magot_fasta_read(tp, size, int(bool(truncate_names)), ctypes.byref(n),
                             ptr(lens), ptr(names), nl.value, ctypes.byref(nl), None, 0),
          'magot_fasta_read')
    return n, lens, names, nl


def fasta_contigs(text, truncate_names=False):
    """(names, lengths) of the contigs the native reader (magot_fasta_read)
    finds in a FASTA text, without copying any sequence; None when a header
    needs the Python reader.  Host only."""
    L = _lib.lib()
    data = _text_view(text)
    idx = _fasta_index(L, _text_ptr(data), len(data), truncate_names)
    if idx is None:
        return None
    n, lens, names, nl = idx
    nms = names[:nl.value].tobytes().split(b'\0')[:n.value]
    return [x.decode('latin-1') for x in nms], [int(x) for x in lens[:n.value]]


def fasta_read(text, truncate_names=False):
    """Native GenomeSequence reader (magot_fasta_read): [(name, bytes)], or None
    when a header needs the Python reader.  Host only."""
    L = _lib.lib()
    data = _text_view(text)
    tp = _text_ptr(data)
    idx = _fasta_index(L, tp, len(data), truncate_names)
    if idx is None:
        return None
    n, lens, names, nl = idx
    seqs = np.zeros(max(int(lens[:n.value].sum()), 1), dtype=np.uint8)
    check(L.magot_fasta_read(tp, len(data), int(bool(truncate_names)), ctypes.byref(n),
                             ptr(lens), ptr(names), nl.value, ctypes.byref(nl), ptr(seqs),
                             len(seqs)), 'magot_fasta_read')
    nms = names[:nl.value].tobytes().split(b'\0')[:n.value]
    out, o = [], 0
    for i in range(n.value):
        out.append((nms[i].decode('latin-1'), seqs[o:o + int(lens[i])].tobytes()))
        o += int(lens[i])
    return out


class FastaGenome(DeviceGenome):
    """A FASTA file read and packed natively (magot_genome_load_fasta): the
    batch path's GenomeSequence, without Python strings.  ``None`` from
    ``load`` when a header needs the Python reader."""

    @classmethod
    def load(cls, text, truncate_names=False, ctx=None):
        L = _lib.lib()
        self = cls.__new__(cls)
        self.ctx = ctx or _lib.default_context()
        self._keepalive = None
        data = _text_view(text)
        h = ctypes.c_void_p()
        rc = L.magot_genome_load_fasta(self.ctx.handle, _text_ptr(data), len(data),
                                       int(bool(truncate_names)), ctypes.byref(h))
        if rc == _lib.ERR_UNSUPPORTED:
            return None
        check(rc, 'magot_genome_load_fasta')
        self.handle = h
        n = ctypes.c_uint32()
        nl = ctypes.c_uint64()
        check(L.magot_genome_contigs(h, ctypes.byref(n), None, None, 0, ctypes.byref(nl)),
              'magot_genome_contigs')
        lens = np.zeros(max(n.value, 1), dtype=np.uint64)
        names = np.zeros(max(nl.value, 1), dtype=np.uint8)
        check(L.magot_genome_contigs(h, ctypes.byref(n), ptr(lens), ptr(names), nl.value,
                                     ctypes.byref(nl)), 'magot_genome_contigs')
        self.names = [x.decode('latin-1') for x in names[:nl.value].tobytes().split(b'\0')[:n.value]]
        self.index = {nm: i for i, nm in enumerate(self.names)}
        self.lengths = lens[:n.value]
        self._stats()
        return self


class ExtractionPlan(object):
    """Interval table -> device plan (magot_plan_create).

    ``exons``: structured array of EXON_DTYPE in output order; ``txs``:
    structured array of TX_DTYPE tiling it.  ``outputs``: OUT_NUC | OUT_PEP,
    optionally | OUT_GENOME_ORDER (records laid out in genome order on the
    device; fetch / copy_outputs still return record order, ``layout()`` gives
    each record's place in the device buffers).
    """

    def __init__(self, genome, exons, txs, outputs=OUT_NUC | OUT_PEP):
        self.genome = genome
        self.ctx = genome.ctx
        exons = np.ascontiguousarray(exons, dtype=EXON_DTYPE)
        txs = np.ascontiguousarray(txs, dtype=TX_DTYPE)
        self.n_exons = len(exons)
        self.n_tx = len(txs)
        self.outputs = outputs
        h = ctypes.c_void_p()
        nb, pb = ctypes.c_uint64(), ctypes.c_uint64()
        check(_lib.lib().magot_plan_create(self.ctx.handle, genome.handle, ptr(exons),
                                           self.n_exons, ptr(txs), self.n_tx, outputs,
                                           ctypes.byref(h), ctypes.byref(nb), ctypes.byref(pb)),
              'magot_plan_create')
        self.handle = h
        self.nuc_bytes = nb.value
        self.pep_bytes = pb.value

    def execute(self):
        check(_lib.lib().magot_plan_execute(self.ctx.handle, self.handle), 'magot_plan_execute')

    def sync(self):
        self.ctx.sync()

    def fetch(self):
        """Returns (nuc uint8[B] or None, nuc_off uint64[T+1], pep uint8[P] or None,
        pep_off uint64[T+1])."""
        nuc = np.empty(self.nuc_bytes, dtype=np.uint8) if self.outputs & OUT_NUC else None
        pep = np.empty(self.pep_bytes, dtype=np.uint8) if self.outputs & OUT_PEP else None
        noff = np.empty(self.n_tx + 1, dtype=np.uint64)
        poff = np.empty(self.n_tx + 1, dtype=np.uint64)
        check(_lib.lib().magot_plan_fetch(self.ctx.handle, self.handle,
                                          ptr(nuc) if nuc is not None and len(nuc) else None,
                                          ptr(noff),
                                          ptr(pep) if pep is not None and len(pep) else None,
                                          ptr(poff)), 'magot_plan_fetch')
        return nuc, noff, pep, poff

    def run(self):
        self.execute()
        return self.fetch()

    def layout(self):
        """(nuc_start uint64[T], pep_start uint64[T]): each record's start in
        the device buffers (magot_plan_layout)."""
        ns = np.empty(self.n_tx, dtype=np.uint64)
        ps = np.empty(self.n_tx, dtype=np.uint64)
        check(_lib.lib().magot_plan_layout(self.handle, ptr(ns) if self.n_tx else None,
                                           ptr(ps) if self.n_tx else None), 'magot_plan_layout')
        return ns, ps

    def copy_outputs(self, nuc_dev_ptr=None, pep_dev_ptr=None):
        """D2D copy of the outputs into caller device memory (addresses)."""
        check(_lib.lib().magot_plan_copy_outputs(
            self.ctx.handle, self.handle,
            ctypes.c_void_p(nuc_dev_ptr) if nuc_dev_ptr else None,
            ctypes.c_void_p(pep_dev_ptr) if pep_dev_ptr else None), 'magot_plan_copy_outputs')

    def fetch_to(self, nuc_addr=None, pep_addr=None):
        """D2H of the outputs straight into caller host memory given by address
        (e.g. pinned buffers); returns (nuc_off, pep_off)."""
        noff = np.empty(self.n_tx + 1, dtype=np.uint64)
        poff = np.empty(self.n_tx + 1, dtype=np.uint64)
        check(_lib.lib().magot_plan_fetch(self.ctx.handle, self.handle,
                                          ctypes.c_void_p(nuc_addr) if nuc_addr else None,
                                          ptr(noff),
                                          ctypes.c_void_p(pep_addr) if pep_addr else None,
                                          ptr(poff)), 'magot_plan_fetch')
        return noff, poff

    def time(self, iters):
        """Mean duration of `iters` isolated launches (an event pair each)."""
        ms = ctypes.c_double()
        check(_lib.lib().magot_plan_time(self.ctx.handle, self.handle, int(iters),
                                         ctypes.byref(ms)), 'magot_plan_time')
        return ms.value

    def time_b2b(self, iters):
        """Per-launch time of `iters` back-to-back launches (one event pair)."""
        ms = ctypes.c_double()
        check(_lib.lib().magot_plan_time_b2b(self.ctx.handle, self.handle, int(iters),
                                             ctypes.byref(ms)), 'magot_plan_time_b2b')
        return ms.value

    @property
    def algorithmic_bytes(self):
        return int(_lib.lib().magot_plan_algorithmic_bytes(self.handle))

    def close(self):
        if getattr(self, 'handle', None):
            _lib.lib().magot_plan_destroy(self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class GffPlan(object):
    """Native gff2fasta planner (magot_gff_plan): GFF text -> interval and
    record tables + FASTA skeleton.  ``GffPlan.build`` returns None when the
    input takes one of the reference's diagnostic paths (the caller then uses
    the object path).  Host-only: no device needed to plan or render."""

    def __init__(self, handle, n_exons, n_tx, protein):
        self.handle = handle
        self.protein = protein
        # the plan's own tables, viewed in place (C3: 72 MB not copied);
        # close() turns the views into copies before the plan goes
        ep, tp = ctypes.c_void_p(), ctypes.c_void_p()
        check(_lib.lib().magot_gffplan_table_views(handle, ctypes.byref(ep), ctypes.byref(tp)),
              'magot_gffplan_table_views')
        self.exons = _view(ep.value, n_exons, EXON_DTYPE)
        self.txs = _view(tp.value, n_tx, TX_DTYPE)
        self._views = True
        n = ctypes.c_uint64()
        check(_lib.lib().magot_gffplan_selections(handle, ctypes.byref(n)),
              'magot_gffplan_selections')
        # longest=True protein choices, made by render() from the peptides
        # (no device text assembly for such a plan)
        self.n_select = n.value

    @classmethod
    def build(cls, gff, names, lengths, feature='gene', protein=False, order='insertion',
              longest=False, genomic=False, from_exons=False):
        """``longest`` / ``genomic``: get_fasta's options (genome.py:677-724).
        genomic=True is never translated (a nucleotide plan whatever
        ``protein`` says).  longest=True over protein candidates is chosen at
        render time (``n_select`` > 0), from the trimmed peptide lengths."""
        L = _lib.lib()
        text = _text_view(gff)
        n = len(names)
        arr = (ctypes.c_char_p * max(n, 1))(*[_as_bytes(x) for x in names])
        lens = np.ascontiguousarray(np.asarray(lengths, dtype=np.uint64))
        flags = (_lib.GFF_PROTEIN if protein else 0) | \
            (_lib.GFF_ORDER_PY2 if order == 'py2' else 0) | \
            (_lib.GFF_LONGEST if longest else 0) | (_lib.GFF_GENOMIC if genomic else 0) | \
            (_lib.GFF_FROM_EXONS if from_exons else 0)
        h = ctypes.c_void_p()
        ne, nt = ctypes.c_uint64(), ctypes.c_uint64()
        rc = L.magot_gff_plan(_text_ptr(text), len(text), arr, lens.ctypes.data_as(_lib._u64p), n,
                              _as_bytes(feature), flags, ctypes.byref(h), ctypes.byref(ne),
                              ctypes.byref(nt))
        if rc == _lib.ERR_UNSUPPORTED:
            return None
        check(rc, 'magot_gff_plan')
        return cls(h, ne.value, nt.value, protein and not genomic)

    @staticmethod
    def flags(protein=False, order='insertion', longest=False, genomic=False, from_exons=False):
        return (_lib.GFF_PROTEIN if protein else 0) | \
            (_lib.GFF_ORDER_PY2 if order == 'py2' else 0) | \
            (_lib.GFF_LONGEST if longest else 0) | (_lib.GFF_GENOMIC if genomic else 0) | \
            (_lib.GFF_FROM_EXONS if from_exons else 0)

    @classmethod
    def flank(cls, gff, names, lengths, sequence_length, stream, feature_type='gene',
              namefrom='ID'):
        """extract_upstream_downstream's windows (genome_tools.py:457-480,
        magot_flank_plan) as a nucleotide plan: one single-interval record per
        printed window, the same skeleton shape as gff2fasta.  None when the
        reference would raise (the caller's line loop reproduces it).
        ``sequence_length`` and ``stream`` are the reference's strings."""
        L = _lib.lib()
        text = _text_view(gff)
        n = len(names)
        arr = (ctypes.c_char_p * max(n, 1))(*[_as_bytes(x) for x in names])
        lens = np.ascontiguousarray(np.asarray(lengths, dtype=np.uint64))
        h = ctypes.c_void_p()
        ne, nt = ctypes.c_uint64(), ctypes.c_uint64()
        rc = L.magot_flank_plan(_text_ptr(text), len(text), arr, lens.ctypes.data_as(_lib._u64p),
                                n, _as_bytes(feature_type), _as_bytes(namefrom),
                                _as_bytes(str(sequence_length)), _as_bytes(stream),
                                ctypes.byref(h), ctypes.byref(ne), ctypes.byref(nt))
        if rc == _lib.ERR_UNSUPPORTED:
            return None
        check(rc, 'magot_flank_plan')
        return cls(h, ne.value, nt.value, False)

    def render(self, nuc, noff, pep, poff):
        """The FASTA text (bytes) around the fetched record payloads."""
        L = _lib.lib()
        size = ctypes.c_uint64()
        args = (ptr(nuc), ptr(noff), ptr(pep), ptr(poff))
        check(L.magot_gffplan_render(self.handle, *args, None, 0, ctypes.byref(size)),
              'magot_gffplan_render')
        out = np.empty(size.value, dtype=np.uint8)
        check(L.magot_gffplan_render(self.handle, *args, ptr(out), size.value,
                                     ctypes.byref(size)), 'magot_gffplan_render')
        return out.tobytes()

    def close(self):
        if self.handle:
            if self._views:
                # the views die with the plan: anyone still holding the
                # attributes keeps valid copies
                self.exons, self.txs = self.exons.copy(), self.txs.copy()
                self._views = False
            _lib.lib().magot_gffplan_destroy(self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def _view(addr, n, dtype):
    """n rows of `dtype` at host address `addr` (not owned; empty when n == 0)."""
    dtype = np.dtype(dtype)
    if not n:
        return np.zeros(0, dtype=dtype)
    buf = (ctypes.c_uint8 * (n * dtype.itemsize)).from_address(addr)
    return np.frombuffer(buf, dtype=dtype, count=n)


class GffRead(object):
    """read_gff done natively (magot_gff_read) before the genome's contigs are
    known; ``lower`` turns it into a GffPlan against them (magot_gff_lower).
    gff2fasta reads the GFF this way while another thread loads the FASTA.
    ``read`` returns None when the input takes a diagnostic path."""

    def __init__(self, handle, text, from_exons):
        self.handle = handle
        self._text = text  # the plan reads views of it until lower() returns
        self.from_exons = from_exons

    @classmethod
    def read(cls, gff, from_exons=False, for_write=False):
        """``for_write``: keep what ``lower_write`` needs (MAGOT_GFF_FOR_WRITE)."""
        L = _lib.lib()
        text = _text_view(gff)
        h = ctypes.c_void_p()
        flags = GffPlan.flags(from_exons=from_exons) | (_lib.GFF_FOR_WRITE if for_write else 0)
        rc = L.magot_gff_read(_text_ptr(text), len(text), flags, ctypes.byref(h))
        if rc == _lib.ERR_UNSUPPORTED:
            if h.value:
                L.magot_gffplan_destroy(h)
            return None
        check(rc, 'magot_gff_read')
        return cls(h, text, from_exons)

    def lower(self, names, lengths, feature='gene', protein=False, order='insertion',
              longest=False, genomic=False):
        """The GffPlan (this object gives its handle up), or None when the
        lowering takes a diagnostic path (the handle is freed)."""
        if not self.handle:
            raise MagotError('GffRead.lower: already lowered or closed')
        L = _lib.lib()
        n = len(names)
        arr = (ctypes.c_char_p * max(n, 1))(*[_as_bytes(x) for x in names])
        lens = np.ascontiguousarray(np.asarray(lengths, dtype=np.uint64))
        flags = GffPlan.flags(protein, order, longest, genomic, self.from_exons)
        ne, nt = ctypes.c_uint64(), ctypes.c_uint64()
        h, self.handle = self.handle, None
        try:
            rc = L.magot_gff_lower(h, arr, lens.ctypes.data_as(_lib._u64p), n, _as_bytes(feature),
                                   flags, ctypes.byref(ne), ctypes.byref(nt))
            if rc == _lib.ERR_UNSUPPORTED:
                return None
            check(rc, 'magot_gff_lower')
            plan = GffPlan(h, ne.value, nt.value, protein and not genomic)
            h = None
            return plan
        finally:
            self._text = None
            if h is not None:
                L.magot_gffplan_destroy(h)

    def lower_cds(self, names, lengths, gene_name_filters=(), gene_length_filter=None,
                  names_from='CDS', order='insertion'):
        """get_CDS_peptides lowered (magot_gff_lower_cds): a CdsPlan with one
        single-interval record per printed CDS in output order, the records'
        names and the transcript groups, or None when anything in the
        annotation takes a diagnostic path.  This object gives its handle up.
        ``gene_name_filters``: strings (a gene whose ID contains one is
        dropped); ``gene_length_filter``: None or an int; ``names_from``: 'CDS',
        'transcript' or 'gene'."""
        if not self.handle:
            raise MagotError('GffRead.lower_cds: already lowered or closed')
        if order not in ('insertion', 'py2'):
            raise ValueError("order must be 'insertion' or 'py2'")
        L = _lib.lib()
        n = len(names)
        arr = (ctypes.c_char_p * max(n, 1))(*[_as_bytes(x) for x in names])
        lens = np.ascontiguousarray(np.asarray(lengths, dtype=np.uint64))
        filters = [_as_bytes(f) for f in gene_name_filters]
        if any(b'\0' in f for f in filters):
            raise ValueError('a filter with a NUL byte')
        farr = (ctypes.c_char_p * max(len(filters), 1))(*filters)
        glf = None if gene_length_filter is None else ctypes.c_int64(int(gene_length_filter))
        nr, ng = ctypes.c_uint64(), ctypes.c_uint64()
        h, self.handle = self.handle, None
        try:
            rc = L.magot_gff_lower_cds(h, arr, lens.ctypes.data_as(_lib._u64p), n, farr,
                                       len(filters), ctypes.byref(glf) if glf is not None else None,
                                       _lib.CDS_NAMES[names_from],
                                       _lib.GFF_ORDER_PY2 if order == 'py2' else 0,
                                       ctypes.byref(nr), ctypes.byref(ng))
            if rc == _lib.ERR_UNSUPPORTED:
                return None
            check(rc, 'magot_gff_lower_cds')
            plan = CdsPlan(h, nr.value, ng.value)
            h = None
            return plan
        finally:
            self._text = None
            if h is not None:
                L.magot_gffplan_destroy(h)

    def lower_write(self, gff_format='simple gff3', order='insertion'):
        """write_gff lowered to output rows (magot_gff_lower_write): a
        GffWritePlan, or None when the walk takes a diagnostic path.  The
        handle stays this object's: any number of formats and orders."""
        if not self.handle:
            raise MagotError('GffRead.lower_write: lowered or closed')
        if order not in ('insertion', 'py2'):
            raise ValueError("order must be 'insertion' or 'py2'")
        L = _lib.lib()
        nr, nb = ctypes.c_uint64(), ctypes.c_uint64()
        rc = L.magot_gff_lower_write(self.handle, _lib.GFF_FORMATS[gff_format],
                                     _lib.GFF_ORDER_PY2 if order == 'py2' else 0,
                                     ctypes.byref(nr), ctypes.byref(nb))
        if rc == _lib.ERR_UNSUPPORTED:
            return None
        check(rc, 'magot_gff_lower_write')
        rows, blob = ctypes.c_void_p(), ctypes.c_void_p()
        check(L.magot_gffplan_write_views(self.handle, ctypes.byref(rows), ctypes.byref(nr),
                                          ctypes.byref(blob), ctypes.byref(nb)),
              'magot_gffplan_write_views')
        return GffWritePlan(self, _view(rows.value, nr.value, _lib.GFFROW_DTYPE),
                            _view(blob.value, nb.value, np.uint8))

    def close(self):
        if self.handle:
            _lib.lib().magot_gffplan_destroy(self.handle)
            self.handle = None
        self._text = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class CdsPlan(object):
    """What GffRead.lower_cds made: ``exons`` / ``txs`` (one single-interval
    record per printed CDS, in output order), ``name_off`` (n + 1) into
    ``names`` (uint8) and ``group_off``: transcript g printed the records
    [group_off[g], group_off[g + 1]).  Copies: the native plan is freed."""

    def __init__(self, handle, n_rec, n_groups):
        L = _lib.lib()
        try:
            ep, tp = ctypes.c_void_p(), ctypes.c_void_p()
            check(L.magot_gffplan_table_views(handle, ctypes.byref(ep), ctypes.byref(tp)),
                  'magot_gffplan_table_views')
            self.exons = _view(ep.value, n_rec, EXON_DTYPE).copy()
            self.txs = _view(tp.value, n_rec, TX_DTYPE).copy()
            no, nm, go = ctypes.c_void_p(), ctypes.c_void_p(), ctypes.c_void_p()
            check(L.magot_gffplan_cds_views(handle, ctypes.byref(no), ctypes.byref(nm),
                                            ctypes.byref(go)), 'magot_gffplan_cds_views')
            self.name_off = _view(no.value, n_rec + 1, np.uint64).copy()
            self.names = _view(nm.value, int(self.name_off[-1]), np.uint8).copy()
            self.group_off = _view(go.value, n_groups + 1, np.uint64).copy()
        finally:
            L.magot_gffplan_destroy(handle)
        self.n_records = n_rec

    def name_list(self):
        raw = self.names.tobytes()
        o = self.name_off
        return [raw[int(o[i]):int(o[i + 1])] for i in range(self.n_records)]


class GffWritePlan(object):
    """The output lines of write_gff as the host planner lowered them: ``rows``
    (GFFROW_DTYPE, one per line, in output order) and ``blob`` (the names the
    planner made up; a reference at or above the GFF text's length points into
    it).  Views of the GffRead's memory: valid until its next ``lower_write``
    or ``close``."""

    def __init__(self, read, rows, blob):
        self._read = read
        self.rows = rows
        self.blob = blob


class GffWriter(object):
    """write_gff's text rendered on the device from a row table
    (magot_gffwrite_*): one lane per row sizes its line, a scan lays the output
    out, one wave per ``params()['rows_per_group']`` rows writes it.  ``parse``
    returns (None, reason, row) where the device declines, ``row`` the first
    offending row counted from 1 (0: none): 'too_large', 'score' (a score
    column outside the two printable classes), 'columns' (a source line
    without eight tabs)."""

    PASSES = ('size', 'scan', 'render', 'copy')

    def __init__(self):
        self.ctx = None
        self.handle = None
        self.n_rows = self.out_bytes = 0
        self.upload_ms = 0.0
        self.declined_row = 0

    @classmethod
    def parse(cls, data, blob, rows, max_bytes=0, ctx=None):
        """``data``: the GFF text; ``blob``: bytes; ``rows``: GFFROW_DTYPE rows
        of any caller.  A row that leaves the text and the blob is a MagotError
        before any launch.  Returns the object, or (None, reason, row) where the
        device declines."""
        self = cls()
        self.ctx = ctx or _lib.default_context()
        view = _text_view(data)
        blob = np.ascontiguousarray(np.frombuffer(bytes(blob), np.uint8)
                                    if isinstance(blob, (bytes, bytearray)) else blob,
                                    dtype=np.uint8).reshape(-1)
        rows = np.ascontiguousarray(rows, dtype=_lib.GFFROW_DTYPE).reshape(-1)
        h, reason, row = ctypes.c_void_p(), ctypes.c_uint32(), ctypes.c_uint64()
        rc = _lib.lib().magot_gffwrite_open(
            self.ctx.handle, _text_ptr(view), len(view), ptr(blob) if len(blob) else None,
            len(blob), ptr(rows) if len(rows) else None, len(rows), int(max_bytes or 0),
            ctypes.byref(h), ctypes.byref(reason), ctypes.byref(row))
        if rc == _lib.ERR_UNSUPPORTED:
            return None, _lib.GFFWRITE_REASONS[reason.value], row.value
        check(rc, 'magot_gffwrite_open')
        self.handle = h
        n, m = ctypes.c_uint64(), ctypes.c_uint64()
        check(_lib.lib().magot_gffwrite_sizes(h, ctypes.byref(n), ctypes.byref(m)),
              'magot_gffwrite_sizes')
        self.n_rows, self.out_bytes = n.value, m.value
        self.upload_ms = float(_lib.lib().magot_gffwrite_upload_ms(h))
        return self

    @staticmethod
    def params():
        """{'rows_per_group': the rows one wave renders, 'threads': the threads
        of a workgroup, 'max_head': the bytes within which a source line's
        eighth tab must lie}"""
        vals = [ctypes.c_uint32() for _ in range(3)]
        _lib.lib().magot_gffwrite_params(*[ctypes.byref(v) for v in vals])
        return dict(zip(('rows_per_group', 'threads', 'max_head'), [v.value for v in vals]))

    def execute(self):
        """The text rendered into the handle's device buffer; its bytes."""
        need = ctypes.c_uint64()
        check(_lib.lib().magot_gffwrite_render(self.ctx.handle, self.handle, ctypes.byref(need)),
              'magot_gffwrite_render')
        return need.value

    def fetch(self, out=None):
        """The rendered text to the host (``out``: a uint8 array to fill)."""
        need = self.out_bytes
        if out is None:
            out = np.empty(max(need, 1), np.uint8)
        check(_lib.lib().magot_gffwrite_render_fetch(self.ctx.handle, self.handle, ptr(out),
                                                     len(out)), 'magot_gffwrite_render_fetch')
        return out[:need]

    def render(self):
        """Every row's line, each ended by LF, as one uint8 array."""
        self.execute()
        return self.fetch()

    def time(self, iters):
        """Mean device ms per pass (PASSES; 'copy': a device copy of 'out_bytes'
        bytes, the render's yardstick) (magot_gffwrite_time)."""
        ms = np.zeros(len(self.PASSES), np.float64)
        n, m = ctypes.c_uint64(), ctypes.c_uint64()
        check(_lib.lib().magot_gffwrite_time(self.ctx.handle, self.handle, int(iters), ptr(ms),
                                             ctypes.byref(n), ctypes.byref(m)),
              'magot_gffwrite_time')
        out = dict(zip(self.PASSES, ms.tolist()))
        out['text_bytes'] = n.value
        out['out_bytes'] = m.value
        return out

    def close(self):
        if getattr(self, 'handle', None):
            _lib.lib().magot_gffwrite_destroy(self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class FastaText(object):
    """The gff2fasta text assembled on device (magot_fasta_text_*): the
    GffPlan skeleton filled with an ExtractionPlan's payloads in one device
    buffer, fetched with a single D2H."""

    def __init__(self, gffplan, extraction):
        L = _lib.lib()
        self.ctx = extraction.ctx
        self._keep = (gffplan, extraction)
        h = ctypes.c_void_p()
        cap = ctypes.c_uint64()
        check(L.magot_fasta_text_create(self.ctx.handle, gffplan.handle, extraction.handle,
                                        ctypes.byref(h), ctypes.byref(cap)),
              'magot_fasta_text_create')
        self.handle = h
        self.max_bytes = cap.value

    def execute(self):
        check(_lib.lib().magot_fasta_text_execute(self.ctx.handle, self.handle),
              'magot_fasta_text_execute')

    def fetch(self):
        """The text as a bytes-like numpy array (no trailing newline)."""
        L = _lib.lib()
        out = np.empty(max(self.max_bytes, 1), dtype=np.uint8)
        n = ctypes.c_uint64()
        check(L.magot_fasta_text_fetch(self.ctx.handle, self.handle, ptr(out), self.max_bytes,
                                       ctypes.byref(n)), 'magot_fasta_text_fetch')
        return out[:n.value]

    def time(self, iters):
        ms = ctypes.c_double()
        check(_lib.lib().magot_fasta_text_time(self.ctx.handle, self.handle, int(iters),
                                               ctypes.byref(ms)), 'magot_fasta_text_time')
        return ms.value

    def close(self):
        if getattr(self, 'handle', None):
            _lib.lib().magot_fasta_text_destroy(self.handle)
            self.handle = None
        self._keep = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def _concat(seqs):
    parts = [_as_bytes(s) for s in seqs]
    off = np.zeros(len(parts) + 1, dtype=np.uint64)
    if parts:
        np.cumsum([len(p) for p in parts], out=off[1:])
    buf = np.frombuffer(b''.join(parts), dtype=np.uint8) if parts else np.zeros(0, np.uint8)
    return buf, off


def revcomp_batch(seqs, ctx=None):
    """Sequence.reverse_compliment (genome.py:784-793) over a list of strings."""
    ctx = ctx or _lib.default_context()
    buf, off = _concat(seqs)
    out = np.empty(max(len(buf), 1), dtype=np.uint8)
    check(_lib.lib().magot_revcomp_batch(ctx.handle, ptr(buf) if len(buf) else None, ptr(off),
                                         len(seqs), ptr(out)), 'magot_revcomp_batch')
    raw = out.tobytes()
    return [raw[int(off[i]):int(off[i + 1])].decode('latin-1') for i in range(len(seqs))]


def orf6_batch(seqs, lut64=None, ctx=None, poison=None, raw=False):
    """The six translations Sequence.get_orfs splits (genome.py:824-851), per
    input: a list of 6 values in the reference's loop order (frame 0,1,2 x
    strand '-','+'), each the trimmed ``translate()`` result or None.

    Test hooks: ``poison`` (a byte value) fills the device output before the
    launch (magot_debug_orf6_batch); ``raw`` returns the untrimmed buffer as
    (padded residue bytes, stream offsets 6n+1, real stream lengths 6n)."""
    ctx = ctx or _lib.default_context()
    n = len(seqs)
    buf, off = _concat(seqs)
    soff = np.empty(6 * n + 1, dtype=np.uint64)
    slen = np.empty(max(6 * n, 1), dtype=np.uint64)
    none = np.empty(max(6 * n, 1), dtype=np.uint8)
    L = _lib.lib()
    check(L.magot_orf6_sizes(ptr(off), n, ptr(soff), ptr(slen), ptr(none)), 'magot_orf6_sizes')
    total = int(soff[6 * n])
    out = np.empty(max(total, 1), dtype=np.uint8)
    lut = np.frombuffer(bytes(lut64), dtype=np.uint8).copy() if lut64 is not None else None
    args = (ctx.handle, ptr(buf) if len(buf) else None, ptr(off), n, ptr(lut), ptr(soff), ptr(out))
    if poison is None:
        check(L.magot_orf6_batch(*args), 'magot_orf6_batch')
    else:
        check(L.magot_debug_orf6_batch(*args, int(poison) & 0xFF), 'magot_debug_orf6_batch')
    if raw:
        return out[:total], soff, slen[:6 * n]
    raw = out[:total].tobytes().decode('latin-1')
    res = []
    for r in range(n):
        six = []
        for j in range(6 * r, 6 * r + 6):
            if none[j]:
                six.append(None)
                continue
            t = raw[int(soff[j]):int(soff[j] + slen[j])]
            if (j % 6) < 2 and t[:1] == 'X':  # frame 0: trimX (genome.py:819-821)
                t = t[1:]
            six.append(t)
        res.append(six)
    return res


class Orf6Plan(object):
    """Six-frame translation of an ExtractionPlan's records, in HBM
    (magot_plan_orf6): BASELINE configs[4] (C5).  The kernel gathers the
    records from the packed genome itself (the plan's nucleotide output is
    neither needed nor read)."""

    def __init__(self, plan, lut64=None):
        self.plan = plan
        self.ctx = plan.ctx
        lut = np.frombuffer(bytes(lut64), dtype=np.uint8).copy() if lut64 is not None else None
        h = ctypes.c_void_p()
        tot = ctypes.c_uint64()
        check(_lib.lib().magot_plan_orf6(self.ctx.handle, plan.handle, ptr(lut), ctypes.byref(h),
                                         ctypes.byref(tot)), 'magot_plan_orf6')
        self.handle = h
        self.total = tot.value

    def execute(self):
        check(_lib.lib().magot_orf6_execute(self.ctx.handle, self.handle), 'magot_orf6_execute')

    def poison(self, byte):
        """Test hook: fill the output with ``byte`` (execute() does not clear it)."""
        check(_lib.lib().magot_orf6_poison(self.ctx.handle, self.handle, int(byte) & 0xFF),
              'magot_orf6_poison')

    def fetch(self):
        """(padded residue bytes, stream offsets 6n+1 (16-aligned), real stream lengths 6n)."""
        out = np.empty(max(self.total, 1), dtype=np.uint8)
        soff = np.empty(6 * self.plan.n_tx + 1, dtype=np.uint64)
        slen = np.empty(max(6 * self.plan.n_tx, 1), dtype=np.uint64)
        check(_lib.lib().magot_orf6_fetch(self.ctx.handle, self.handle, ptr(out), ptr(soff),
                                          ptr(slen)), 'magot_orf6_fetch')
        return out[:self.total], soff, slen[:6 * self.plan.n_tx]

    def fetch_to(self, out_addr):
        """D2H of the padded residue bytes into caller host memory (an address,
        e.g. a pinned buffer of ``total`` bytes); returns (stream_off, stream_len)."""
        soff = np.empty(6 * self.plan.n_tx + 1, dtype=np.uint64)
        slen = np.empty(max(6 * self.plan.n_tx, 1), dtype=np.uint64)
        check(_lib.lib().magot_orf6_fetch(self.ctx.handle, self.handle,
                                          ctypes.c_void_p(out_addr) if out_addr else None,
                                          ptr(soff), ptr(slen)), 'magot_orf6_fetch')
        return soff, slen[:6 * self.plan.n_tx]

    def copy_outputs(self, dst_dev_ptr):
        """D2D copy of the padded residue bytes (``total``) into caller device
        memory (an address), e.g. the buffer an output gather sends."""
        check(_lib.lib().magot_orf6_copy_outputs(self.ctx.handle, self.handle,
                                                 ctypes.c_void_p(dst_dev_ptr)),
              'magot_orf6_copy_outputs')

    def time(self, iters):
        ms = ctypes.c_double()
        check(_lib.lib().magot_orf6_time(self.ctx.handle, self.handle, int(iters),
                                         ctypes.byref(ms)), 'magot_orf6_time')
        return ms.value

    def time_b2b(self, iters):
        ms = ctypes.c_double()
        check(_lib.lib().magot_orf6_time_b2b(self.ctx.handle, self.handle, int(iters),
                                             ctypes.byref(ms)), 'magot_orf6_time_b2b')
        return ms.value

    def close(self):
        if getattr(self, 'handle', None):
            _lib.lib().magot_orf6_destroy(self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


# Residues per tile of the ORF-calling passes (kOrfCallTile, orfcall.hip;
# magot_orfcall_tile() is checked against it): an ORF may span any number.
ORFCALL_TILE = 1024

ORF_TABLE_DTYPE = np.dtype([('record', '<u4'), ('stream', 'u1'), ('start', '<u4'),
                            ('length', '<u4'), ('payload_off', '<u8')])


class OrfCalls(object):
    """ORFs called on the device from an executed Orf6Plan's streams
    (magot_orfcall_*): dna2orfs (genome_tools.py:145-180) over the plan's
    records.  ``table()`` gives one row per ORF (``longest``: per unflagged
    record) in record order and the reference's loop order inside a record
    (stream j = 2*frame + (strand == '+')), the concatenated output strings
    and a flag byte per record (_lib.ORF_REC_NONE: a stream whose translate()
    is None; _lib.ORF_REC_NO_LONGEST: no longest candidate).  ``text(names)``
    gives the tool's FASTA text, assembled on the device."""

    def __init__(self, orf6plan, from_atg=False, longest=False):
        L = _lib.lib()
        if L.magot_orfcall_tile() != ORFCALL_TILE:
            raise MagotError('ORFCALL_TILE does not match the library')
        self.ctx = orf6plan.ctx
        self._keep = orf6plan
        self.n_records = orf6plan.plan.n_tx
        self.from_atg, self.longest = bool(from_atg), bool(longest)
        flags = (_lib.ORF_FROM_ATG if from_atg else 0) | (_lib.ORF_LONGEST if longest else 0)
        h = ctypes.c_void_p()
        n, pb = ctypes.c_uint64(), ctypes.c_uint64()
        check(L.magot_orfcall_create(self.ctx.handle, orf6plan.handle, flags, ctypes.byref(h),
                                     ctypes.byref(n), ctypes.byref(pb)), 'magot_orfcall_create')
        self.handle = h
        self.n_orfs = n.value
        self.payload_bytes = pb.value

    def table(self):
        """(rows ORF_TABLE_DTYPE[n_orfs], payload uint8[payload_bytes], record
        flags uint8[n_records])."""
        n = self.n_orfs
        rec = np.empty(max(n, 1), np.uint32)
        st = np.empty(max(n, 1), np.uint8)
        k = np.empty(max(n, 1), np.uint32)
        ln = np.empty(max(n, 1), np.uint32)
        po = np.empty(max(n, 1), np.uint64)
        pay = np.empty(max(self.payload_bytes, 1), np.uint8)
        fl = np.zeros(max(self.n_records, 1), np.uint8)
        check(_lib.lib().magot_orfcall_fetch(self.ctx.handle, self.handle, ptr(rec), ptr(st),
                                             ptr(k), ptr(ln), ptr(po), ptr(pay), ptr(fl)),
              'magot_orfcall_fetch')
        rows = np.empty(n, ORF_TABLE_DTYPE)
        rows['record'], rows['stream'], rows['start'] = rec[:n], st[:n], k[:n]
        rows['length'], rows['payload_off'] = ln[:n], po[:n]
        return rows, pay[:self.payload_bytes], fl[:self.n_records]

    def flags(self):
        """The flag byte of every record."""
        fl = np.zeros(max(self.n_records, 1), np.uint8)
        check(_lib.lib().magot_orfcall_fetch(self.ctx.handle, self.handle, None, None, None,
                                             None, None, None, ptr(fl)), 'magot_orfcall_fetch')
        return fl[:self.n_records]

    def text(self, names):
        """The FASTA text (a uint8 array) for one name per record (str or
        bytes, any bytes): '>name-pos:P\nORF\n' per ORF, or with ``longest``
        '>name_longestORF\nORF\n' per unflagged record."""
        if len(names) != self.n_records:
            raise ValueError('one name per record')
        buf, off = _concat(names)
        size = ctypes.c_uint64()
        L = _lib.lib()
        check(L.magot_orfcall_text(self.ctx.handle, self.handle, ptr(off),
                                   ptr(buf) if len(buf) else None, ctypes.byref(size)),
              'magot_orfcall_text')
        out = np.empty(max(size.value, 1), np.uint8)
        check(L.magot_orfcall_text_fetch(self.ctx.handle, self.handle, ptr(out), size.value),
              'magot_orfcall_text_fetch')
        return out[:size.value]

    def time(self, iters, text=False):
        """Mean device time (ms) of the calling passes, or with ``text`` of the
        text passes of the last ``text()`` call."""
        ms = ctypes.c_double()
        check(_lib.lib().magot_orfcall_time(self.ctx.handle, self.handle, int(bool(text)),
                                            int(iters), ctypes.byref(ms)), 'magot_orfcall_time')
        return ms.value

    def close(self):
        if getattr(self, 'handle', None):
            _lib.lib().magot_orfcall_destroy(self.handle)
            self.handle = None
        self._keep = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


LONGORF_TABLE_DTYPE = np.dtype([('stream', 'u1'), ('start', '<u4'), ('length', '<u4'),
                                ('payload_off', '<u8')])


class LongestOrfs(object):
    """The longest six-frame ORF of every record of an executed ExtractionPlan
    with OUT_NUC (magot_longorf_*): Sequence.get_orfs(longest=True)
    (genome.py:824-851) over the plan's nucleotide output where it lies in
    HBM, in one fused pass that writes no stream and no losing ORF.
    ``table()`` gives one row per record in record order (stream j = 2*frame +
    (strand == '+'), start residue, length, payload offset), the concatenated
    winners and a flag byte per record (_lib.ORF_REC_NO_LONGEST: no candidate,
    the reference's IndexError; its row has length 0).  ``text(names,
    n_print)`` gives '>name\\nORF\\n' for the first ``n_print`` records,
    assembled on the device."""

    def __init__(self, plan, lut64=None):
        self.ctx = plan.ctx
        self._keep = plan
        self.n_records = plan.n_tx
        lut = np.frombuffer(bytes(lut64), dtype=np.uint8).copy() if lut64 is not None else None
        if lut is not None and len(lut) != 64:
            raise ValueError('lut64 holds 64 residues')
        L = _lib.lib()
        h = ctypes.c_void_p()
        check(L.magot_longorf_create(self.ctx.handle, plan.handle, ptr(lut), ctypes.byref(h)),
              'magot_longorf_create')
        self.handle = h
        pb = ctypes.c_uint64()
        check(L.magot_longorf_execute(self.ctx.handle, h, ctypes.byref(pb)),
              'magot_longorf_execute')
        self.payload_bytes = pb.value

    def table(self):
        """(rows LONGORF_TABLE_DTYPE[n_records], payload uint8[payload_bytes],
        record flags uint8[n_records])."""
        n = self.n_records
        st = np.empty(max(n, 1), np.uint8)
        k = np.empty(max(n, 1), np.uint32)
        ln = np.empty(max(n, 1), np.uint32)
        po = np.empty(max(n, 1), np.uint64)
        pay = np.empty(max(self.payload_bytes, 1), np.uint8)
        fl = np.zeros(max(n, 1), np.uint8)
        check(_lib.lib().magot_longorf_fetch(self.ctx.handle, self.handle, ptr(st), ptr(k),
                                             ptr(ln), ptr(po), ptr(pay), ptr(fl)),
              'magot_longorf_fetch')
        rows = np.empty(n, LONGORF_TABLE_DTYPE)
        rows['stream'], rows['start'] = st[:n], k[:n]
        rows['length'], rows['payload_off'] = ln[:n], po[:n]
        return rows, pay[:self.payload_bytes], fl[:n]

    def flags(self):
        """The flag byte of every record."""
        fl = np.zeros(max(self.n_records, 1), np.uint8)
        check(_lib.lib().magot_longorf_fetch(self.ctx.handle, self.handle, None, None, None,
                                             None, None, ptr(fl)), 'magot_longorf_fetch')
        return fl[:self.n_records]

    def text(self, names, n_print=None):
        """The text (a uint8 array) '>name\\nORF\\n' of records [0, n_print)
        (all of them by default) for one name per record (str or bytes)."""
        if len(names) != self.n_records:
            raise ValueError('one name per record')
        n_print = self.n_records if n_print is None else int(n_print)
        if not 0 <= n_print <= self.n_records:
            raise ValueError('n_print outside [0, records]')
        buf, off = _concat(names[:n_print])
        return self.text_blob(buf, off, n_print)

    def text_blob(self, buf, off, n_print):
        """``text`` with the names as a uint8 blob and uint64 offsets
        (``n_print`` + 1 of them at least)."""
        buf = np.ascontiguousarray(buf, dtype=np.uint8)
        off = np.ascontiguousarray(off, dtype=np.uint64)
        if not 0 <= n_print <= self.n_records or len(off) < n_print + 1 or \
                (n_print and int(off[n_print]) > len(buf)):
            raise ValueError('n_print or the name table does not fit')
        size = ctypes.c_uint64()
        L = _lib.lib()
        check(L.magot_longorf_text(self.ctx.handle, self.handle, ptr(off),
                                   ptr(buf) if len(buf) else None, n_print, ctypes.byref(size)),
              'magot_longorf_text')
        out = np.empty(max(size.value, 1), np.uint8)
        check(L.magot_longorf_text_fetch(self.ctx.handle, self.handle, ptr(out), size.value),
              'magot_longorf_text_fetch')
        return out[:size.value]

    def time(self, iters, text=False):
        """Mean device time (ms) of the calling passes, or with ``text`` of the
        text passes of the last ``text()`` call."""
        ms = ctypes.c_double()
        check(_lib.lib().magot_longorf_time(self.ctx.handle, self.handle, int(bool(text)),
                                            int(iters), ctypes.byref(ms)), 'magot_longorf_time')
        return ms.value

    def params(self):
        """{'step': codons per step of the calling pass, 'waves': waves this
        handle launches, 'max_waves': the most any handle of the context does}."""
        L = _lib.lib()
        step, w, mw = ctypes.c_uint32(), ctypes.c_uint64(), ctypes.c_uint64()
        check(L.magot_longorf_params(self.ctx.handle, self.handle, ctypes.byref(step),
                                     ctypes.byref(w)), 'magot_longorf_params')
        check(L.magot_longorf_params(self.ctx.handle, None, None, ctypes.byref(mw)),
              'magot_longorf_params')
        return {'step': step.value, 'waves': w.value, 'max_waves': mw.value}

    def close(self):
        if getattr(self, 'handle', None):
            _lib.lib().magot_longorf_destroy(self.handle)
            self.handle = None
        self._keep = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


MASK_INTERVAL_DTYPE = _lib.MASK_INTERVAL_DTYPE


def mask_fasta_check(text, n_contigs):
    """True when the ``n_contigs`` contigs the native reader found in the
    FASTA ``text`` (truncate_names) are the entries mask_from_gff's own read
    loop builds (magot_mask_fasta_check, genome_tools.py:398-409).  Host only."""
    data = _text_view(text)
    rc = _lib.lib().magot_mask_fasta_check(_text_ptr(data), len(data), int(n_contigs))
    if rc == _lib.ERR_UNSUPPORTED:
        return False
    check(rc, 'magot_mask_fasta_check')
    return True


class MaskPlan(object):
    """mask_from_gff's GFF pass as an interval table (magot_mask_plan,
    genome_tools.py:410-426): ``intervals`` holds MASK_INTERVAL_DTYPE pieces
    {contig, 0-based start, len} of at most ``piece`` bases, in GFF order,
    clipped, unsorted and unmerged.  ``MaskPlan.build`` returns None where
    only the reference's sequential replay is exact (the caller's line loop).
    Host only."""

    def __init__(self, handle, hard, keep_case):
        self.handle = handle
        self.hard, self.keep_case = hard, keep_case
        rows, n = ctypes.c_void_p(), ctypes.c_uint64()
        check(_lib.lib().magot_maskplan_table(handle, ctypes.byref(rows), ctypes.byref(n), None),
              'magot_maskplan_table')
        self.intervals = _view(rows.value, n.value, MASK_INTERVAL_DTYPE).copy()
        self.piece = int(_lib.lib().magot_mask_piece())

    @classmethod
    def build(cls, gff, names, lengths, feature_type='CDS', hard=False, keep_case=False):
        L = _lib.lib()
        text = _text_view(gff)
        n = len(names)
        arr = (ctypes.c_char_p * max(n, 1))(*[_as_bytes(x) for x in names])
        lens = np.ascontiguousarray(np.asarray(lengths, dtype=np.uint64))
        flags = (_lib.MASK_HARD if hard else 0) | (_lib.MASK_KEEP_CASE if keep_case else 0)
        h = ctypes.c_void_p()
        rc = L.magot_mask_plan(_text_ptr(text), len(text), arr, lens.ctypes.data_as(_lib._u64p),
                               n, _as_bytes(feature_type), flags, ctypes.byref(h), None)
        if rc == _lib.ERR_UNSUPPORTED:
            return None
        check(rc, 'magot_mask_plan')
        return cls(h, bool(hard), bool(keep_case))

    def close(self):
        if getattr(self, 'handle', None):
            _lib.lib().magot_maskplan_destroy(self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def whole_contig_plan(genome, contigs):
    """An ExtractionPlan gathering the contigs ``contigs`` (indices) of a
    device genome whole, one '+' single-interval nucleotide record each."""
    idx = np.asarray(contigs, dtype=np.int64)
    ex = np.zeros(len(idx), dtype=EXON_DTYPE)
    ex['contig'] = idx
    ex['len'] = np.asarray(genome.lengths, dtype=np.uint64)[idx]
    tx = np.zeros(len(idx), dtype=TX_DTYPE)
    tx['exon_begin'] = np.arange(len(idx))
    tx['n_exons'] = 1
    return ExtractionPlan(genome, ex, tx, OUT_NUC)


class GenomeMask(object):
    """mask_from_gff's text built on the device (magot_mask_*,
    genome_tools.py:394-428): ``extraction`` gathers every contig whole, one
    record per contig in output order (``whole_contig_plan``); record r is
    contig ``rec_contig[r]`` and is printed under ``names[r]``.  ``execute``
    enqueues the coverage paint and the text pass behind the extraction;
    ``fetch`` gives the text, ``coverage()`` the coverage plane (one bit per
    byte of the extraction's output; ``extraction.layout()`` places the
    records in it)."""

    def __init__(self, extraction, maskplan, rec_contig, names):
        if len(names) != extraction.n_tx or len(rec_contig) != extraction.n_tx:
            raise ValueError('one name and one contig per record')
        self.ctx = extraction.ctx
        self._keep = extraction
        rc_arr = np.ascontiguousarray(np.asarray(rec_contig, dtype=np.uint32))
        buf, off = _concat(names)
        h = ctypes.c_void_p()
        tb = ctypes.c_uint64()
        check(_lib.lib().magot_mask_create(self.ctx.handle, extraction.handle, maskplan.handle,
                                           ptr(rc_arr) if len(rc_arr) else None, ptr(off),
                                           ptr(buf) if len(buf) else None, ctypes.byref(h),
                                           ctypes.byref(tb)), 'magot_mask_create')
        self.handle = h
        self.text_bytes = tb.value

    def execute(self):
        check(_lib.lib().magot_mask_execute(self.ctx.handle, self.handle), 'magot_mask_execute')

    def fetch(self):
        """The text (a uint8 array): '>' name '\\n' sequence '\\n' per record."""
        out = np.empty(max(self.text_bytes, 1), np.uint8)
        check(_lib.lib().magot_mask_fetch(self.ctx.handle, self.handle, ptr(out),
                                          self.text_bytes), 'magot_mask_fetch')
        return out[:self.text_bytes]

    def coverage(self):
        """The coverage plane as uint32 words (bit i of word w: byte 32 w + i
        of the extraction's nucleotide output)."""
        n = ctypes.c_uint64()
        L = _lib.lib()
        check(L.magot_mask_coverage_fetch(self.ctx.handle, self.handle, None, 0, ctypes.byref(n)),
              'magot_mask_coverage_fetch')
        words = np.zeros(max(n.value, 1), np.uint32)
        check(L.magot_mask_coverage_fetch(self.ctx.handle, self.handle, ptr(words), n.value,
                                          ctypes.byref(n)), 'magot_mask_coverage_fetch')
        return words[:n.value]

    def time(self, iters):
        """(paint_ms, text_ms): mean device time of the plane's zeroing +
        paint kernel and of the text kernel (magot_mask_time)."""
        pm, tm = ctypes.c_double(), ctypes.c_double()
        check(_lib.lib().magot_mask_time(self.ctx.handle, self.handle, int(iters),
                                         ctypes.byref(pm), ctypes.byref(tm)), 'magot_mask_time')
        return pm.value, tm.value

    def close(self):
        if getattr(self, 'handle', None):
            _lib.lib().magot_mask_destroy(self.handle)
            self.handle = None
        self._keep = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def interval_pieces(contig, start, length, piece):
    """Intervals {contig, 0-based start, length} (arrays) cut into
    MASK_INTERVAL_DTYPE rows of at most ``piece`` bases; empty ones dropped."""
    contig = np.asarray(contig, dtype=np.int64)
    start = np.asarray(start, dtype=np.int64)
    length = np.asarray(length, dtype=np.int64)
    n = (length + piece - 1) // piece
    which = np.repeat(np.arange(len(n)), n)
    k = np.arange(int(n.sum())) - np.repeat(np.cumsum(n) - n, n)
    rows = np.zeros(len(which), dtype=MASK_INTERVAL_DTYPE)
    rows['contig'] = contig[which]
    rows['start'] = start[which] + k * piece
    rows['len'] = np.minimum(length[which] - k * piece, piece)
    return rows


def _interval_rows(contig, start, length):
    rows = np.zeros(len(contig), dtype=MASK_INTERVAL_DTYPE)
    rows['contig'], rows['start'], rows['len'] = contig, start, length
    return rows


class TrackWindows(object):
    """The sliding-window sums of a GenomeTrack, resident on the device
    (magot_track_windows_create): ``first[c]`` is contig c's first window of
    ``n_windows``; ``sums()`` brings them all down, ``transitions(s_min)``
    only the windows where ``sum >= s_min`` flips."""

    def __init__(self, track, window, jump, skip=None):
        self.ctx = track.ctx
        self._keep = track
        nc = len(track.genome.names)
        sk = None
        if skip is not None:
            sk = np.ascontiguousarray(np.asarray(skip, dtype=bool).astype(np.uint8))
            if len(sk) != nc:
                raise ValueError('one skip flag per contig')
        self.first = np.zeros(nc + 1, dtype=np.uint64)
        h, n = ctypes.c_void_p(), ctypes.c_uint64()
        check(_lib.lib().magot_track_windows_create(
            self.ctx.handle, track.handle, int(window), int(jump),
            ptr(sk) if sk is not None and nc else None, ctypes.byref(h), ctypes.byref(n),
            ptr(self.first)), 'magot_track_windows_create')
        self.handle = h
        self.n_windows = n.value
        self.window, self.jump = int(window), int(jump)

    def sums(self):
        out = np.empty(max(self.n_windows, 1), np.uint32)
        check(_lib.lib().magot_track_windows_fetch(self.ctx.handle, self.handle, ptr(out),
                                                   self.n_windows), 'magot_track_windows_fetch')
        return out[:self.n_windows]

    def transitions(self, s_min):
        """Ascending window indices where ``sum >= s_min`` differs from the
        previous window of the same contig (false before its first)."""
        n = ctypes.c_uint64()
        L = _lib.lib()
        check(L.magot_track_transitions(self.ctx.handle, self.handle, int(s_min), ctypes.byref(n)),
              'magot_track_transitions')
        out = np.empty(max(n.value, 1), np.uint64)
        check(L.magot_track_transitions_fetch(self.ctx.handle, self.handle, ptr(out), n.value),
              'magot_track_transitions_fetch')
        return out[:n.value]

    def close(self):
        if getattr(self, 'handle', None):
            _lib.lib().magot_track_windows_destroy(self.handle)
            self.handle = None
        self._keep = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class GenomeTrack(object):
    """position_dic's per-base track on the device (magot_track_*,
    genome.py:981-1100): one bit per base of a DeviceGenome.  Producers:
    ``base_class`` (A/T or C/G content), ``paint`` (intervals), ``set_bytes``
    (a contig's bool array).  Consumers: ``get_bytes``, ``count``
    (ones under intervals), ``windows`` (TrackWindows: sums and threshold
    transitions).  genome -> base_class -> windows -> transitions never brings
    anything per base to the host."""

    def __init__(self, genome):
        if not isinstance(genome, DeviceGenome):
            raise MagotError('GenomeTrack needs a genome in one device plane')
        self.ctx = genome.ctx
        self.genome = genome
        h, n = ctypes.c_void_p(), ctypes.c_uint64()
        check(_lib.lib().magot_track_create(self.ctx.handle, genome.handle, ctypes.byref(h),
                                            ctypes.byref(n)), 'magot_track_create')
        self.handle = h
        self.n_words = n.value
        self.piece = int(_lib.lib().magot_mask_piece())

    def base_class(self, gc=False, replace=False, genome=None):
        """OR the A/T (``gc``: C/G) class of the genome's bases into the track,
        or replace the track with it."""
        g = self.genome if genome is None else genome
        flags = (_lib.TRACK_GC if gc else 0) | (_lib.TRACK_REPLACE if replace else 0)
        check(_lib.lib().magot_track_base_class(self.ctx.handle, self.handle, g.handle, flags),
              'magot_track_base_class')

    def paint(self, contig, start, length, value=1):
        """Set (``value`` 1) or clear (0) the bases of every interval."""
        rows = interval_pieces(contig, start, length, self.piece)
        self.paint_rows(rows, value)

    def paint_rows(self, rows, value=1):
        rows = np.ascontiguousarray(rows, dtype=MASK_INTERVAL_DTYPE)
        check(_lib.lib().magot_track_paint(self.ctx.handle, self.handle,
                                           ptr(rows) if len(rows) else None, len(rows),
                                           int(value)), 'magot_track_paint')

    def set_bytes(self, contig, arr):
        a = np.ascontiguousarray(arr).view(np.uint8).reshape(-1)
        check(_lib.lib().magot_track_set_bytes(self.ctx.handle, self.handle, int(contig),
                                               ptr(a) if len(a) else None, len(a)),
              'magot_track_set_bytes')

    def get_bytes(self, contig, out=None):
        """The contig's bits as a bool array (into ``out``, a contiguous bool
        or uint8 array of the contig's length, when given)."""
        n = int(self.genome.lengths[contig])
        if out is None:
            out = np.empty(n, dtype=bool)
        a = out.view(np.uint8).reshape(-1)
        check(_lib.lib().magot_track_get_bytes(self.ctx.handle, self.handle, int(contig),
                                               ptr(a) if len(a) else None, len(a)),
              'magot_track_get_bytes')
        return out

    def words(self):
        out = np.zeros(max(self.n_words, 1), np.uint32)
        check(_lib.lib().magot_track_fetch(self.ctx.handle, self.handle, ptr(out), self.n_words,
                                           None), 'magot_track_fetch')
        return out[:self.n_words]

    def count(self, contig, start, length):
        """Ones under each interval (any length), a uint32 array."""
        return self.count_rows(_interval_rows(contig, start, length))

    def count_rows(self, rows):
        rows = np.ascontiguousarray(rows, dtype=MASK_INTERVAL_DTYPE)
        out = np.zeros(max(len(rows), 1), np.uint32)
        check(_lib.lib().magot_track_count(self.ctx.handle, self.handle,
                                           ptr(rows) if len(rows) else None, len(rows), ptr(out)),
              'magot_track_count')
        return out[:len(rows)]

    def windows(self, window, jump=1, skip=None):
        return TrackWindows(self, window, jump, skip)

    def time(self, iters, windows=None, s_min=1):
        """Mean device ms per pass: {'class', 'rank', 'windows', 'transitions',
        'count'} (magot_track_time)."""
        ms = np.zeros(5, np.float64)
        check(_lib.lib().magot_track_time(self.ctx.handle, self.handle,
                                          windows.handle if windows is not None else None,
                                          int(s_min), int(iters), ptr(ms)), 'magot_track_time')
        return dict(zip(('class', 'rank', 'windows', 'transitions', 'count'), ms.tolist()))

    def close(self):
        if getattr(self, 'handle', None):
            _lib.lib().magot_track_destroy(self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class DepthTrack(object):
    """depth_from_gff's per-base track on the device (magot_depth_*,
    genome_tools.py:598-652): the depth column of a ``samtools depth`` table
    as one int32 per line.  For a table inside the native grammar (magot.h)
    every contig is one run of lines with positions 1, 2, ..: ``names``,
    ``lengths`` and ``first`` (the run's first line) are the contig table,
    and the reference's array of a contig is lines [first, first + length).

    ``parse`` always returns a track; one with ``declined == (reason,
    line_no)`` (the first offending line, 1-based; None for a whole-table
    limit) holds nothing else."""

    def __init__(self):
        self.ctx = None
        self.handle = None
        self.declined = None
        self.names, self.index = [], {}
        self.lengths = self.first = np.zeros(0, np.int64)
        self.n_lines = 0
        self.block = int(_lib.lib().magot_depth_block())

    @classmethod
    def parse(cls, buffer, chunk_bytes=None, max_runs=None, ctx=None):
        """The table in ``buffer`` (bytes, mmap, numpy), streamed to the device
        in chunks of about ``chunk_bytes`` (default: sized for transfer)."""
        self = cls()
        self.ctx = ctx or _lib.default_context()
        view = _text_view(buffer)
        h = ctypes.c_void_p()
        n_lines, n_runs, line = ctypes.c_uint64(), ctypes.c_uint64(), ctypes.c_uint64()
        reason = ctypes.c_uint32()
        check(_lib.lib().magot_depth_parse(self.ctx.handle, _text_ptr(view), len(view),
                                           int(chunk_bytes or 0), int(max_runs or 0),
                                           ctypes.byref(h), ctypes.byref(n_lines),
                                           ctypes.byref(n_runs), ctypes.byref(reason),
                                           ctypes.byref(line)), 'magot_depth_parse')
        if reason.value:
            self.declined = (_lib.DEPTH_REASONS[reason.value], line.value or None)
            return self
        self.handle = h
        self.n_lines = n_lines.value
        n = n_runs.value
        first = np.zeros(max(n, 1), np.uint64)
        offset = np.zeros(max(n, 1), np.uint64)
        name_len = np.zeros(max(n, 1), np.uint32)
        check(_lib.lib().magot_depth_runs(self.handle, ptr(first), ptr(offset), ptr(name_len), n),
              'magot_depth_runs')
        self.first = first[:n].astype(np.int64)
        self.lengths = np.diff(np.append(self.first, self.n_lines))
        self.names = [view[o:o + k].tobytes().decode('latin-1')
                      for o, k in zip(offset[:n].tolist(), name_len[:n].tolist())]
        self.index = {nm: i for i, nm in enumerate(self.names)}
        return self

    def _contig(self, contig):
        return self.index[contig] if isinstance(contig, str) else int(contig)

    def values(self, contig):
        """An int32 copy of one contig's depths (for tests)."""
        c = self._contig(contig)
        out = np.zeros(max(int(self.lengths[c]), 1), np.int32)
        check(_lib.lib().magot_depth_values(self.ctx.handle, self.handle, int(self.first[c]),
                                            int(self.lengths[c]), ptr(out)), 'magot_depth_values')
        return out[:int(self.lengths[c])]

    def _rows(self, contig, start, length):
        c = np.asarray(contig, dtype=np.int64).reshape(-1)
        s = np.ascontiguousarray(self.first[c] + np.asarray(start, dtype=np.int64).reshape(-1))
        return s, np.ascontiguousarray(np.asarray(length, dtype=np.int64).reshape(-1))

    def sums(self, contig, start, length):
        """int64 sum of each interval: ``length`` depths from 0-based ``start``
        of contig (index) ``contig``; a length <= 0 gives 0.  The caller clips
        to the contig, as a numpy slice does."""
        return self.group_sums(contig, start, length, None)[0]

    def group_sums(self, contig, start, length, group_offsets):
        """(sums, group sums): ``group_offsets`` is a CSR over the rows
        (n_groups + 1 ascending row indices)."""
        s, ln = self._rows(contig, start, length)
        if len(s) != len(ln):
            raise MagotError('DepthTrack: one start and one length per row')
        out = np.zeros(max(len(s), 1), np.int64)
        off = groups = None
        n_groups = 0
        if group_offsets is not None:
            off = np.ascontiguousarray(group_offsets, dtype=np.uint64)
            n_groups = len(off) - 1
            groups = np.zeros(max(n_groups, 1), np.int64)
        check(_lib.lib().magot_depth_sums(self.ctx.handle, self.handle,
                                          ptr(s) if len(s) else None, ptr(ln) if len(s) else None,
                                          len(s), ptr(off) if n_groups > 0 else None,
                                          max(n_groups, 0), ptr(out),
                                          ptr(groups) if n_groups > 0 else None),
              'magot_depth_sums')
        return out[:len(s)], (None if groups is None else groups[:max(n_groups, 0)])

    def time(self, iters):
        """Mean device ms per pass: {'line_index', 'parse', 'directory',
        'sums'}, the first two over the last chunk ('chunk_bytes' bytes of
        text), the others over the whole table (magot_depth_time)."""
        ms = np.zeros(4, np.float64)
        n = ctypes.c_uint64()
        check(_lib.lib().magot_depth_time(self.ctx.handle, self.handle, int(iters), ptr(ms),
                                          ctypes.byref(n)), 'magot_depth_time')
        out = dict(zip(('line_index', 'parse', 'directory', 'sums'), ms.tolist()))
        out['chunk_bytes'] = n.value
        return out

    def close(self):
        if getattr(self, 'handle', None):
            _lib.lib().magot_depth_destroy(self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class ReadLengths(object):
    """fqstats' read lengths on the device (magot_fq_*, genome_tools.py:85-124):
    the lengths of a FASTQ's sequence lines -- line k (from 0) with k % 4 == 1,
    ended by LF only, whatever they hold -- as a histogram, and the tool's
    figures reduced from it there.  Lines may be of any length and the text is
    cut into chunks anywhere; nothing is declined."""

    KEYS = ('reads', 'bases', 'median', 'reads25', 'reads75', 'n25', 'n50', 'n75')

    def __init__(self):
        self.ctx = None
        self.handle = None
        self.reads = self.bases = 0
        self.dense = int(_lib.lib().magot_fq_dense())
        self._stats = None

    @classmethod
    def parse(cls, data, chunk_bytes=0, ctx=None):
        """The FASTQ text in ``data`` (bytes, a buffer, an mmap, numpy), streamed
        to the device in chunks of ``chunk_bytes`` (0: sized for transfer)."""
        self = cls()
        self.ctx = ctx or _lib.default_context()
        view = _text_view(data)
        h = ctypes.c_void_p()
        check(_lib.lib().magot_fq_parse(self.ctx.handle, _text_ptr(view), len(view),
                                        int(chunk_bytes or 0), ctypes.byref(h)), 'magot_fq_parse')
        self.handle = h
        out = np.zeros(8, np.uint64)
        flags = ctypes.c_uint32()
        check(_lib.lib().magot_fq_stats(self.handle, ptr(out), ctypes.byref(flags)),
              'magot_fq_stats')
        vals = [int(x) for x in out.tolist()]
        for k in range(3):  # an N-value that was never set
            if not flags.value >> k & 1:
                vals[5 + k] = None
        self._stats = dict(zip(self.KEYS, vals))
        self.reads, self.bases = vals[0], vals[1]
        return self

    def stats(self):
        """{'reads', 'bases', 'median', 'reads25', 'reads75', 'n25', 'n50',
        'n75'}: the figures fqstats prints, in its order; an N-value that was
        never set (no bases at all) is None.  With no reads the order
        statistics mean nothing (the tool divides by zero before them)."""
        return dict(self._stats)

    def histogram(self):
        """(lengths ascending, int64 counts): the lengths that occur."""
        n = ctypes.c_uint64()
        L = _lib.lib()
        check(L.magot_fq_histogram(self.ctx.handle, self.handle, None, None, 0, ctypes.byref(n)),
              'magot_fq_histogram')
        lengths = np.zeros(max(n.value, 1), np.int64)
        counts = np.zeros(max(n.value, 1), np.uint64)
        check(L.magot_fq_histogram(self.ctx.handle, self.handle, ptr(lengths), ptr(counts),
                                   n.value, ctypes.byref(n)), 'magot_fq_histogram')
        return lengths[:n.value], counts[:n.value].astype(np.int64)

    def time(self, iters):
        """Mean device ms per pass: {'line_index', 'lengths', 'reduce', 'copy'},
        the first two and the device copy over the last chunk ('chunk_bytes'
        bytes of text), the reduction over the whole histogram (magot_fq_time)."""
        ms = np.zeros(4, np.float64)
        n = ctypes.c_uint64()
        check(_lib.lib().magot_fq_time(self.ctx.handle, self.handle, int(iters), ptr(ms),
                                       ctypes.byref(n)), 'magot_fq_time')
        out = dict(zip(('line_index', 'lengths', 'reduce', 'copy'), ms.tolist()))
        out['chunk_bytes'] = n.value
        return out

    def close(self):
        if getattr(self, 'handle', None):
            _lib.lib().magot_fq_destroy(self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def _query_columns(seq, c0, c1):
    """(uint32 seqids, int64 c0, int64 c1) of equal length for the ABI; a
    seqid below zero becomes OVERLAP_NO_SEQ (no partner)."""
    seq = np.asarray(seq, dtype=np.int64).reshape(-1)
    seq = np.where((seq < 0) | (seq >= _lib.OVERLAP_NO_SEQ), _lib.OVERLAP_NO_SEQ, seq)
    seq = np.ascontiguousarray(seq.astype(np.uint32))
    c0 = np.ascontiguousarray(np.asarray(c0, dtype=np.int64).reshape(-1))
    c1 = np.ascontiguousarray(np.asarray(c1, dtype=np.int64).reshape(-1))
    if not len(seq) == len(c0) == len(c1):
        raise ValueError('seq, start and end must have one entry per interval')
    return seq, c0, c1


class IntervalIndex(object):
    """One set of intervals (dense seqid, start, end) sorted on the device for
    the reference's two interval joins (magot_overlap_*; genome_tools.py:548-568,
    annotation_funcs.py:13-30).  The integers are taken as they are: reversed
    and negative coordinates are legal, nothing is clipped; they must lie in
    ``coord_range()``.  Queries name their seqid by the same dense numbers; one
    the index does not hold (negative, or beyond the largest) has no partner."""

    PASSES = ('keys', 'sort', 'segments', 'purge', 'overlap', 'copy')

    def __init__(self, seq, start, end, n_seq=None, ctx=None):
        self.ctx = ctx or _lib.default_context()
        self.handle = None
        seq = np.asarray(seq, dtype=np.int64).reshape(-1)
        if len(seq) and (seq.min() < 0 or seq.max() >= _lib.OVERLAP_NO_SEQ):
            raise ValueError('seqids of the index must be dense numbers from 0')
        seq, p0, p1 = _query_columns(seq, start, end)
        self.n = len(seq)
        self.n_seq = int(n_seq) if n_seq is not None else (int(seq.max()) + 1 if self.n else 0)
        h = ctypes.c_void_p()
        check(_lib.lib().magot_overlap_create(self.ctx.handle, ptr(seq), ptr(p0), ptr(p1), self.n,
                                              self.n_seq, ctypes.byref(h)), 'magot_overlap_create')
        self.handle = h

    @staticmethod
    def coord_range():
        """(lowest, highest) coordinate an index or a query may hold."""
        lo, hi = ctypes.c_int64(), ctypes.c_int64()
        _lib.lib().magot_overlap_coord_range(ctypes.byref(lo), ctypes.byref(hi))
        return lo.value, hi.value

    @staticmethod
    def lane_scan():
        """overlap_counts' range scan: a query with more intervals starting
        inside it than this is scanned by a whole wave, not by its lane."""
        return int(_lib.lib().magot_overlap_lane_scan())

    def purge_flags(self, seq, c0, c1):
        """purge_overlaps' test per query, a bool array: True where an interval
        p of the query's seqid has p0 < c0 < p1, p0 < c1 < p1 or c0 < p0 < c1."""
        seq, c0, c1 = _query_columns(seq, c0, c1)
        out = np.zeros(max(len(seq), 1), np.uint8)
        check(_lib.lib().magot_overlap_purge(self.ctx.handle, self.handle, ptr(seq), ptr(c0),
                                             ptr(c1), len(seq), ptr(out)), 'magot_overlap_purge')
        return out[:len(seq)].astype(bool)

    def overlap_counts(self, seq, q0, q1):
        """annotation_overlap's partners per query, int64: the intervals p of
        the query's seqid with p0 <= q0 <= p1 or p0 <= q1 <= p1."""
        seq, q0, q1 = _query_columns(seq, q0, q1)
        out = np.zeros(max(len(seq), 1), np.int64)
        check(_lib.lib().magot_overlap_counts(self.ctx.handle, self.handle, ptr(seq), ptr(q0),
                                              ptr(q1), len(seq), ptr(out)), 'magot_overlap_counts')
        return out[:len(seq)]

    def time(self, iters):
        """Mean device ms per pass: {'keys', 'sort', 'segments'} of the index
        build, {'purge', 'overlap'} over the last query set given to either
        method (0 when none was), and 'copy', a device copy of the sorted tables
        ('copy_bytes' bytes) (magot_overlap_time)."""
        ms = np.zeros(6, np.float64)
        n = ctypes.c_uint64()
        check(_lib.lib().magot_overlap_time(self.ctx.handle, self.handle, int(iters), ptr(ms),
                                            ctypes.byref(n)), 'magot_overlap_time')
        out = dict(zip(self.PASSES, ms.tolist()))
        out['copy_bytes'] = n.value
        return out

    def close(self):
        if getattr(self, 'handle', None):
            _lib.lib().magot_overlap_destroy(self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class OverlapPlan(object):
    """purge_overlaps' two GFF texts as tables (magot_overlap_plan,
    genome_tools.py:548-568), a row per line: ``tables[k]`` for file k holds
    'flag' (more than 6 tabs), 'seq' (dense seqid in the first file's
    dictionary; OVERLAP_NO_SEQ where the second file's seqid is not there, or
    no flag), 'c0', 'c1', 'off', 'len'.  ``OverlapPlan.build`` returns
    (None, reason) where only the reference's sequential run is exact.  Host
    only."""

    COLUMNS = (('flag', np.uint8), ('seq', np.uint32), ('c0', np.int64), ('c1', np.int64),
               ('off', np.uint64), ('len', np.uint64))

    def __init__(self, handle, second):
        self.handle = handle
        self._second = second  # the text render() copies from
        self.tables = []
        L = _lib.lib()
        for which in (0, 1):
            n, n_seq = ctypes.c_uint64(), ctypes.c_uint32()
            cols = [ctypes.c_void_p() for _ in self.COLUMNS]
            check(L.magot_ovplan_table(handle, which, ctypes.byref(n), ctypes.byref(n_seq),
                                       *[ctypes.byref(c) for c in cols]), 'magot_ovplan_table')
            self.n_seq = n_seq.value
            self.tables.append({name: _view(c.value, n.value, dt)
                                for (name, dt), c in zip(self.COLUMNS, cols)})

    @classmethod
    def build(cls, gff1, gff2):
        first, second = _text_view(gff1), _text_view(gff2)
        h, reason = ctypes.c_void_p(), ctypes.c_uint32()
        rc = _lib.lib().magot_overlap_plan(_text_ptr(first), len(first), _text_ptr(second),
                                           len(second), ctypes.byref(h), ctypes.byref(reason))
        if rc == _lib.ERR_UNSUPPORTED:
            return None, _lib.OVERLAP_REASONS[reason.value]
        check(rc, 'magot_overlap_plan')
        return cls(h, second), None

    def render(self, drop):
        """The second file's lines with ``drop[line]`` false, each without its
        last byte and with LF instead, in file order (a uint8 array)."""
        drop = np.ascontiguousarray(np.asarray(drop, dtype=np.uint8))
        if len(drop) != len(self.tables[1]['flag']):
            raise ValueError('one flag per line of the second file')
        L = _lib.lib()
        n = ctypes.c_uint64()
        text = self._second
        check(L.magot_ovplan_render(self.handle, _text_ptr(text), len(text),
                                    ptr(drop) if len(drop) else None, None, 0, ctypes.byref(n)),
              'magot_ovplan_render')
        out = np.empty(max(n.value, 1), np.uint8)
        check(L.magot_ovplan_render(self.handle, _text_ptr(text), len(text),
                                    ptr(drop) if len(drop) else None, ptr(out), n.value,
                                    ctypes.byref(n)), 'magot_ovplan_render')
        return out[:n.value]

    def close(self):
        if getattr(self, 'handle', None):
            self.tables = []
            _lib.lib().magot_ovplan_destroy(self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class BestHits(object):
    """besthits_from_psl's keyed reduction on the device (magot_psl_*,
    genome_tools.py:572-592): per query name of a PSL text -- the bytes between
    a data line's 9th tab and the next tab or the line's end -- the line with
    the highest field 0 - field 1, the earliest among equals.  Lines are
    grouped by CPython 2.7's string hash of the key, sorted, and every group is
    verified byte for byte; ``parse`` returns (None, reason) where only the
    line loop is exact: 'few_fields', 'integer_form', 'number_range' (a data
    line outside the native grammar), 'hash_collision', 'too_large',
    'too_many_lines'."""

    PASSES = ('line_index', 'parse', 'compact', 'sort', 'verify', 'reduce', 'order', 'copy')
    GROUP_COLUMNS = (('hash', np.uint64), ('first_line', np.uint32), ('best_line', np.uint32),
                     ('score', np.int64), ('off', np.uint64), ('len', np.uint64))

    def __init__(self):
        self.ctx = None
        self.handle = None
        self.n_lines = self.n_pass = self.n_data = self.n_groups = 0
        self.upload_ms = 0.0

    @classmethod
    def parse(cls, data, hash_bits=64, max_bytes=0, ctx=None):
        """The PSL text in ``data`` (bytes, a buffer, an mmap, numpy) made
        resident on the device and reduced.  ``hash_bits``: the low bits of the
        hash the lines are grouped by (two keys in one bucket decline the text;
        fewer than 64 bits only serve to test that).  ``max_bytes``: a longer
        text is declined (0: a quarter of the free device memory)."""
        self = cls()
        self.ctx = ctx or _lib.default_context()
        view = _text_view(data)
        h, reason, line = ctypes.c_void_p(), ctypes.c_uint32(), ctypes.c_uint64()
        rc = _lib.lib().magot_psl_parse(self.ctx.handle, _text_ptr(view), len(view),
                                        int(hash_bits), int(max_bytes or 0), ctypes.byref(h),
                                        ctypes.byref(reason), ctypes.byref(line))
        if rc == _lib.ERR_UNSUPPORTED:
            return None, _lib.PSL_REASONS[reason.value]
        check(rc, 'magot_psl_parse')
        self.handle = h
        sizes = [ctypes.c_uint64() for _ in range(4)]
        check(_lib.lib().magot_psl_sizes(h, *[ctypes.byref(x) for x in sizes]), 'magot_psl_sizes')
        self.n_lines, self.n_pass, self.n_data, self.n_groups = [x.value for x in sizes]
        # device ms of the upload, the staging copies on the host included
        self.upload_ms = float(_lib.lib().magot_psl_upload_ms(h))
        return self

    def pass_lines(self):
        """(off, len) of the pass-through lines in file order, uint64 each; a
        length counts the line's LF."""
        off = np.zeros(max(self.n_pass, 1), np.uint64)
        length = np.zeros(max(self.n_pass, 1), np.uint64)
        check(_lib.lib().magot_psl_pass_lines(self.ctx.handle, self.handle, ptr(off), ptr(length)),
              'magot_psl_pass_lines')
        return off[:self.n_pass], length[:self.n_pass]

    def groups(self):
        """One row per key in first-seen order, as a dict of arrays: 'hash'
        (the key's full 64-bit hash), 'first_line', 'best_line' (0-based),
        'score', and 'off', 'len' of the best line (its LF counted)."""
        cols = [np.zeros(max(self.n_groups, 1), dt) for _, dt in self.GROUP_COLUMNS]
        check(_lib.lib().magot_psl_groups(self.ctx.handle, self.handle, *[ptr(c) for c in cols]),
              'magot_psl_groups')
        return {name: c[:self.n_groups] for (name, _), c in zip(self.GROUP_COLUMNS, cols)}

    def time(self, iters):
        """Mean device ms per pass (PASSES; 'copy': a device copy of the text,
        'text_bytes' bytes) (magot_psl_time)."""
        ms = np.zeros(len(self.PASSES), np.float64)
        n = ctypes.c_uint64()
        check(_lib.lib().magot_psl_time(self.ctx.handle, self.handle, int(iters), ptr(ms),
                                        ctypes.byref(n)), 'magot_psl_time')
        out = dict(zip(self.PASSES, ms.tolist()))
        out['text_bytes'] = n.value
        return out

    def close(self):
        if getattr(self, 'handle', None):
            _lib.lib().magot_psl_destroy(self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def py2_order_of_hashes(hashes):
    """The order (indices, uint64) in which a CPython 2.7 dict iterates distinct
    keys inserted in the given order, from their string hashes alone
    (magot_psl_order; py2order.dict_order on the host, natively)."""
    hashes = np.ascontiguousarray(np.asarray(hashes, dtype=np.uint64).reshape(-1))
    perm = np.zeros(max(len(hashes), 1), np.uint64)
    check(_lib.lib().magot_psl_order(ptr(hashes) if len(hashes) else None, len(hashes), ptr(perm)),
          'magot_psl_order')
    return perm[:len(hashes)]


def render_lines(data, off, length, whole=False):
    """The rows (off, length) of the text in ``data``, each without its last
    byte and with LF instead (``whole``: all of it and an LF), as one uint8
    array (magot_psl_render)."""
    view = _text_view(data)
    off = np.ascontiguousarray(np.asarray(off, dtype=np.uint64).reshape(-1))
    length = np.ascontiguousarray(np.asarray(length, dtype=np.uint64).reshape(-1))
    if len(off) != len(length):
        raise ValueError('one length per offset')
    n, need = len(off), ctypes.c_uint64()
    L = _lib.lib()
    args = (_text_ptr(view), len(view), ptr(off) if n else None, ptr(length) if n else None, n,
            1 if whole else 0)
    check(L.magot_psl_render(*args, None, 0, ctypes.byref(need)), 'magot_psl_render')
    out = np.empty(max(need.value, 1), np.uint8)
    check(L.magot_psl_render(*args, ptr(out), need.value, ctypes.byref(need)), 'magot_psl_render')
    return out[:need.value]


class FastaRecords(object):
    """The records of a FASTA text on the device (magot_fastarec_*;
    genome.py:854-877, genome_tools.py:377-391, magot_smallfuncs.py:21-29): a
    line index, a line table that reads two bytes of every line however long
    it is, one lane per header for the name and its CPython 2.7 hash, the
    records with a sequence grouped by name as a dict keeps them (a sort by
    hash, every group verified byte for byte), an anti-join of the keys against
    a list of names, and the text reflowed into one line per record.  ``parse``
    returns (None, reason) where only the host loop is exact: 'leading_text',
    'stray_cr', 'long_name', 'hash_collision', 'too_large', 'too_many_lines';
    ``declined_line`` then holds the 1-based line (0: the whole text)."""

    PASSES = ('line_index', 'line_table', 'names', 'sort', 'keys', 'reflow', 'copy')
    RECORD_COLUMNS = (('line', np.uint32), ('name_off', np.uint64), ('name_len', np.uint32),
                      ('seq_len', np.uint64), ('hash', np.uint64), ('word_off', np.uint64),
                      ('word_len', np.uint32), ('word_hash', np.uint64), ('no_word', np.uint32))
    KEY_COLUMNS = (('hash', np.uint64), ('first_record', np.uint32), ('last_record', np.uint32),
                   ('no_word', np.uint32))
    declined_line = 0  # of the last declined parse

    def __init__(self):
        self.ctx = None
        self.handle = None
        self.n_lines = self.n_records = self.n_with_sequence = self.n_keys = 0
        self.upload_ms = 0.0

    @classmethod
    def parse(cls, data, hash_bits=64, max_bytes=0, ctx=None):
        """The FASTA text in ``data`` (bytes, a buffer, an mmap, numpy) made
        resident on the device, indexed and grouped.  ``hash_bits``: the low
        bits of the hash the records are grouped by and the names of a list are
        looked up by (two keys in one bucket decline the text; fewer than 64
        bits only serve to test that).  ``max_bytes``: a longer text is
        declined (0: a quarter of the free device memory)."""
        self = cls()
        self.ctx = ctx or _lib.default_context()
        view = _text_view(data)
        h, reason, line = ctypes.c_void_p(), ctypes.c_uint32(), ctypes.c_uint64()
        rc = _lib.lib().magot_fastarec_parse(self.ctx.handle, _text_ptr(view), len(view),
                                             int(hash_bits), int(max_bytes or 0), ctypes.byref(h),
                                             ctypes.byref(reason), ctypes.byref(line))
        if rc == _lib.ERR_UNSUPPORTED:
            cls.declined_line = line.value
            return None, _lib.FASTAREC_REASONS[reason.value]
        check(rc, 'magot_fastarec_parse')
        self.handle = h
        sizes = [ctypes.c_uint64() for _ in range(4)]
        check(_lib.lib().magot_fastarec_sizes(h, *[ctypes.byref(x) for x in sizes]),
              'magot_fastarec_sizes')
        self.n_lines, self.n_records, self.n_with_sequence, self.n_keys = [x.value for x in sizes]
        self.upload_ms = float(_lib.lib().magot_fastarec_upload_ms(h))
        return self

    @staticmethod
    def params():
        """{'max_name': the longest name in bytes, 'piece': the bytes of a
        sequence line one lane slot of the reflow copies, 'text_block': the
        bytes per workgroup of the line index}"""
        vals = [ctypes.c_uint32() for _ in range(3)]
        _lib.lib().magot_fastarec_params(*[ctypes.byref(v) for v in vals])
        return dict(zip(('max_name', 'piece', 'text_block'), [v.value for v in vals]))

    def records(self):
        """One row per header line in file order, as a dict of arrays: 'line'
        (0-based), 'name_off', 'name_len', 'seq_len', 'hash' (of the name), and
        the first word's 'word_off', 'word_len', 'word_hash' with 'no_word'."""
        cols = [np.zeros(max(self.n_records, 1), dt) for _, dt in self.RECORD_COLUMNS]
        check(_lib.lib().magot_fastarec_records(self.ctx.handle, self.handle,
                                                *[ptr(c) for c in cols]), 'magot_fastarec_records')
        return {name: c[:self.n_records] for (name, _), c in zip(self.RECORD_COLUMNS, cols)}

    def keys(self):
        """One row per dict key in first-seen order: 'hash', 'first_record' (its
        place), 'last_record' (its sequence), 'no_word'."""
        cols = [np.zeros(max(self.n_keys, 1), dt) for _, dt in self.KEY_COLUMNS]
        check(_lib.lib().magot_fastarec_keys(self.ctx.handle, self.handle, *[ptr(c) for c in cols]),
              'magot_fastarec_keys')
        return {name: c[:self.n_keys] for (name, _), c in zip(self.KEY_COLUMNS, cols)}

    def exclude(self, names, first_word=False):
        """A bool array over the keys: False where the key (its first word with
        ``first_word``; the empty word where it has none) is one of ``names``
        (byte strings)."""
        names = [n.encode('latin-1') if isinstance(n, str) else bytes(n) for n in names]
        blob = np.frombuffer(b''.join(names), np.uint8)
        off = np.zeros(len(names) + 1, np.uint64)
        if names:
            off[1:] = np.cumsum([len(n) for n in names], dtype=np.uint64)
        keep = np.ones(max(self.n_keys, 1), np.uint8)
        check(_lib.lib().magot_fastarec_exclude(self.ctx.handle, self.handle,
                                                ptr(blob) if len(blob) else None, len(blob),
                                                ptr(off), len(names), 1 if first_word else 0,
                                                ptr(keep)), 'magot_fastarec_exclude')
        return keep[:self.n_keys].astype(bool)

    def render(self, records, style):
        """The records (indices into ``records()``) in the order given as one
        uint8 array: ``style`` 'fasta' ('>' name LF sequence LF) or 'tab' (name
        TAB sequence, an LF between records and one at the end)."""
        recs = np.ascontiguousarray(np.asarray(records, dtype=np.uint32).reshape(-1))
        need = ctypes.c_uint64()
        check(_lib.lib().magot_fastarec_render(self.ctx.handle, self.handle,
                                               ptr(recs) if len(recs) else None, len(recs),
                                               _lib.FASTAREC_STYLES[style], ctypes.byref(need)),
              'magot_fastarec_render')
        out = np.empty(max(need.value, 1), np.uint8)
        check(_lib.lib().magot_fastarec_render_fetch(self.ctx.handle, self.handle, ptr(out),
                                                     need.value), 'magot_fastarec_render_fetch')
        return out[:need.value]

    def time(self, iters):
        """Mean device ms per pass (PASSES; 'reflow': every record in file
        order in the 'tab' style, 'reflow_bytes' of output; 'copy': a device copy
        of the text, 'text_bytes' bytes) (magot_fastarec_time)."""
        ms = np.zeros(len(self.PASSES), np.float64)
        n, m = ctypes.c_uint64(), ctypes.c_uint64()
        check(_lib.lib().magot_fastarec_time(self.ctx.handle, self.handle, int(iters), ptr(ms),
                                             ctypes.byref(n), ctypes.byref(m)),
              'magot_fastarec_time')
        out = dict(zip(self.PASSES, ms.tolist()))
        out['text_bytes'] = n.value
        out['reflow_bytes'] = m.value
        return out

    def close(self):
        if getattr(self, 'handle', None):
            _lib.lib().magot_fastarec_destroy(self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def _blob_of(items):
    """(the byte strings joined as a uint8 array, their len + 1 offsets)"""
    off = np.zeros(len(items) + 1, np.uint64)
    if items:
        off[1:] = np.cumsum([len(x) for x in items], dtype=np.uint64)
    return np.frombuffer(b''.join(items), np.uint8), off


def py2_string_hashes(keys):
    """CPython 2.7's string hash (py2order.str_hash) of every byte string of
    ``keys`` as a uint64 array: one numpy pass per byte position, over the keys
    that long."""
    blob, off = _blob_of(keys)
    length = np.diff(off)
    h = np.zeros(len(keys), np.uint64)
    live = np.flatnonzero(length)
    h[live] = blob[off[live].astype(np.int64)].astype(np.uint64) << np.uint64(7)
    with np.errstate(over='ignore'):
        for i in range(int(length.max()) if len(keys) else 0):
            live = live[length[live] > i]
            c = blob[(off[live] + np.uint64(i)).astype(np.int64)].astype(np.uint64)
            h[live] = (h[live] * np.uint64(1000003)) ^ c
    h ^= length
    h[h == np.uint64(0xFFFFFFFFFFFFFFFF)] = np.uint64(0xFFFFFFFFFFFFFFFE)
    h[length == 0] = 0
    return h


class NameReplacer(object):
    """replace_names over a resident text (magot_rename_*;
    genome_tools.py:431-446): the words a table names, each ending at the
    one-byte delimiter ``d``, replaced by the table's values.  The names go into
    an open-addressing table keyed by a hash taken from a name's last byte to
    its first; one lane per ``d`` of the text walks left over at most the
    longest name, probes at every length the table has, compares the bytes of a
    hash hit and keeps the hit of lowest rank; a scan lays the output out and a
    grouped copy writes it.  Exact where no name and no value holds ``d`` and no
    key's value feeds a later key: genome_tools.replace_names checks that.
    ``parse`` returns (None, reason) where the device declines: 'too_large',
    'hash_collision', 'table_too_large'."""

    PASSES = ('table', 'field_ends', 'match', 'layout', 'render', 'copy')

    def __init__(self):
        self.ctx = None
        self.handle = None
        self.n_lines = self.n_fields = self.n_hits = self.out_bytes = 0
        self.upload_ms = 0.0

    @classmethod
    def parse(cls, data, names, values, d, ranks=None, hash_bits=64, max_bytes=0, ctx=None):
        """The text in ``data`` (bytes, a buffer, an mmap, numpy) made resident
        and matched against the table: ``names`` distinct byte strings of 1 to
        ``params()['max_name']`` bytes, ``values`` one byte string each, ``d``
        the delimiter (one byte, not LF), ``ranks`` each name's place in the
        order the reference tries the keys (default: as listed).  ``hash_bits``:
        the low bits of the hash the names are looked up by (two names in one
        bucket decline the call; fewer than 64 bits only serve to test that).
        ``max_bytes``: a longer text is declined (0: a quarter of the free
        device memory)."""
        self = cls()
        self.ctx = ctx or _lib.default_context()
        view = _text_view(data)
        names, values = [bytes(x) for x in names], [bytes(x) for x in values]
        if len(values) != len(names):
            raise ValueError('one value per name')
        if isinstance(d, str):
            d = d.encode('latin-1')
        if len(d) != 1:
            raise ValueError('the delimiter is one byte')
        rank = np.ascontiguousarray(np.arange(len(names)) if ranks is None else ranks,
                                    dtype=np.uint32).reshape(-1)
        if len(rank) != len(names):
            raise ValueError('one rank per name')
        name_blob, name_off = _blob_of(names)
        val_blob, val_off = _blob_of(values)
        h, reason = ctypes.c_void_p(), ctypes.c_uint32()
        rc = _lib.lib().magot_rename_parse(
            self.ctx.handle, _text_ptr(view), len(view), _text_ptr(name_blob), ptr(name_off),
            _text_ptr(val_blob), ptr(val_off), ptr(rank) if len(rank) else None, len(names), d[0],
            int(hash_bits), int(max_bytes or 0), ctypes.byref(h), ctypes.byref(reason))
        if rc == _lib.ERR_UNSUPPORTED:
            return None, _lib.RENAME_REASONS[reason.value]
        check(rc, 'magot_rename_parse')
        self.handle = h
        sizes = [ctypes.c_uint64() for _ in range(4)]
        check(_lib.lib().magot_rename_sizes(h, *[ctypes.byref(x) for x in sizes]),
              'magot_rename_sizes')
        self.n_lines, self.n_fields, self.n_hits, self.out_bytes = [x.value for x in sizes]
        self.upload_ms = float(_lib.lib().magot_rename_upload_ms(h))
        return self

    @staticmethod
    def params():
        """{'max_name': the longest name in bytes, 'text_block': the bytes per
        workgroup of the field index, 'piece': the bytes of an unchanged run one
        lane slot of the copy takes}"""
        vals = [ctypes.c_uint32() for _ in range(3)]
        _lib.lib().magot_rename_params(*[ctypes.byref(v) for v in vals])
        return dict(zip(('max_name', 'text_block', 'piece'), [v.value for v in vals]))

    def hits(self):
        """The rewritten fields in text order, as a dict of arrays: 'end' (the
        offset of the field's delimiter) and 'key' (the index of the name)."""
        end = np.zeros(max(self.n_hits, 1), np.uint64)
        key = np.zeros(max(self.n_hits, 1), np.uint32)
        check(_lib.lib().magot_rename_hits(self.ctx.handle, self.handle, ptr(end), ptr(key)),
              'magot_rename_hits')
        return {'end': end[:self.n_hits], 'key': key[:self.n_hits]}

    def render(self):
        """What the reference prints, as one uint8 array."""
        need = ctypes.c_uint64()
        check(_lib.lib().magot_rename_render(self.ctx.handle, self.handle, ctypes.byref(need)),
              'magot_rename_render')
        out = np.empty(max(need.value, 1), np.uint8)
        check(_lib.lib().magot_rename_render_fetch(self.ctx.handle, self.handle, ptr(out),
                                                   need.value), 'magot_rename_render_fetch')
        return out[:need.value]

    def time(self, iters):
        """Mean device ms per pass (PASSES; 'render': the copy into the output,
        'out_bytes' bytes; 'copy': a device copy of the text, 'text_bytes' bytes)
        (magot_rename_time)."""
        ms = np.zeros(len(self.PASSES), np.float64)
        n, m = ctypes.c_uint64(), ctypes.c_uint64()
        check(_lib.lib().magot_rename_time(self.ctx.handle, self.handle, int(iters), ptr(ms),
                                           ctypes.byref(n), ctypes.byref(m)), 'magot_rename_time')
        out = dict(zip(self.PASSES, ms.tolist()))
        out['text_bytes'] = n.value
        out['out_bytes'] = m.value
        return out

    def close(self):
        if getattr(self, 'handle', None):
            _lib.lib().magot_rename_destroy(self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class TabCut(object):
    """A column cut of a resident tab-separated text (magot_tabcut_*;
    magot_smallfuncs.py:12-18, genome_tools.py:449-454): for every line a few
    leading fields taken by their TAB positions and printed with literals
    between them.  A program is ``need`` (the TABs a line must have),
    ``short`` ('skip' or 'error': what a line with fewer does), ``cr_check``
    and its items: a byte string is a literal, a pair ``(a, b)`` the source
    bytes of the fields a..b, inner TABs included.  The LFs and the TABs are
    indexed in one pass; one lane per line finds its TABs by a search and lays
    the line out, one lane per 4 KiB piece names a copy, and a grouped copy
    writes the text: no lane walks a field.  ``parse`` returns (None, reason)
    where the device declines: 'stray_cr', 'too_large', 'too_many_lines'."""

    PASSES = ('index', 'rows', 'layout', 'pieces', 'render', 'copy')
    TAB2FASTA = dict(need=1, short='error', cr_check=True,
                     items=(b'>', (0, 0), b'\n', (1, 1), b'\n'))
    HINTS = dict(need=6, short='skip', cr_check=False,
                 items=((0, 1), b'\tnonexonpart\t', (3, 5), b'\t.\t.\tpri=2;src=RM\n'))

    def __init__(self):
        self.ctx = None
        self.handle = None
        self.n_lines = self.n_tabs = self.n_kept = self.n_pieces = self.out_bytes = 0
        self.short_line = None  # the lowest short line of 'error' (0-based), None when none
        self.upload_ms = 0.0

    @staticmethod
    def lower(items):
        """(the magot_tabcut_item rows, the literal blob) of a program's items"""
        rows = np.zeros(len(items), _lib.TABCUT_ITEM_DTYPE)
        blob = bytearray()
        for row, item in zip(rows, items):
            if isinstance(item, (bytes, bytearray)):
                row['kind'], row['a'], row['b'] = _lib.TABCUT_LITERAL, len(blob), len(item)
                blob += item
            else:
                row['kind'], row['a'], row['b'] = _lib.TABCUT_FIELDS, item[0], item[1]
        return rows, np.frombuffer(bytes(blob), np.uint8)

    @classmethod
    def parse(cls, data, need, short, items, cr_check=False, max_bytes=0, ctx=None):
        """The text in ``data`` (bytes, a buffer, an mmap, numpy) made resident,
        indexed and laid out under the program.  ``max_bytes``: a longer text is
        declined (0: a quarter of the free device memory).  A short line under
        'error' is no decline: ``short_line`` names the lowest."""
        self = cls()
        self.ctx = ctx or _lib.default_context()
        view = _text_view(data)
        rows, blob = cls.lower(items)
        return self._open(view, rows, blob, need, _lib.TABCUT_SHORT[short], cr_check, max_bytes)

    def _open(self, view, rows, blob, need, short_mode, cr_check, max_bytes):
        h, reason = ctypes.c_void_p(), ctypes.c_uint32()
        rc = _lib.lib().magot_tabcut_parse(
            self.ctx.handle, _text_ptr(view), len(view), ptr(rows) if len(rows) else None,
            len(rows), _text_ptr(blob), len(blob), int(need), int(short_mode),
            1 if cr_check else 0, int(max_bytes or 0), ctypes.byref(h), ctypes.byref(reason))
        if rc == _lib.ERR_UNSUPPORTED:
            return None, _lib.TABCUT_REASONS[reason.value]
        check(rc, 'magot_tabcut_parse')
        self.handle = h
        sizes = [ctypes.c_uint64() for _ in range(6)]
        check(_lib.lib().magot_tabcut_sizes(h, *[ctypes.byref(x) for x in sizes]),
              'magot_tabcut_sizes')
        (self.n_lines, self.n_tabs, self.n_kept, self.n_pieces, self.out_bytes,
         short_line) = [x.value for x in sizes]
        self.short_line = None if short_line == 2 ** 64 - 1 else short_line
        self.upload_ms = float(_lib.lib().magot_tabcut_upload_ms(h))
        return self

    @staticmethod
    def params():
        """{'piece': the bytes of an item one lane slot of the copy takes,
        'text_block': the bytes per workgroup of the indexes, 'max_items': the
        most items of a program}"""
        vals = [ctypes.c_uint32() for _ in range(3)]
        _lib.lib().magot_tabcut_params(*[ctypes.byref(v) for v in vals])
        return dict(zip(('piece', 'text_block', 'max_items'), [v.value for v in vals]))

    def rows(self):
        """Per line, as a dict of arrays: 'verdict' (0 skipped, 1 kept, 2
        short under 'error') and 'offset' (where its output begins)."""
        verdict = np.zeros(max(self.n_lines, 1), np.uint8)
        offset = np.zeros(max(self.n_lines, 1), np.uint64)
        check(_lib.lib().magot_tabcut_rows(self.ctx.handle, self.handle, ptr(verdict),
                                           ptr(offset)), 'magot_tabcut_rows')
        return {'verdict': verdict[:self.n_lines], 'offset': offset[:self.n_lines]}

    def render(self):
        """What the kept lines print, as one uint8 array."""
        need = ctypes.c_uint64()
        check(_lib.lib().magot_tabcut_render(self.ctx.handle, self.handle, ctypes.byref(need)),
              'magot_tabcut_render')
        out = np.empty(max(need.value, 1), np.uint8)
        check(_lib.lib().magot_tabcut_render_fetch(self.ctx.handle, self.handle, ptr(out),
                                                   need.value), 'magot_tabcut_render_fetch')
        return out[:need.value]

    def time(self, iters):
        """Mean device ms per pass (PASSES; 'render': the copy into the output,
        'out_bytes' bytes; 'copy': a device copy of the text, 'text_bytes' bytes)
        (magot_tabcut_time)."""
        ms = np.zeros(len(self.PASSES), np.float64)
        n, m = ctypes.c_uint64(), ctypes.c_uint64()
        check(_lib.lib().magot_tabcut_time(self.ctx.handle, self.handle, int(iters), ptr(ms),
                                           ctypes.byref(n), ctypes.byref(m)), 'magot_tabcut_time')
        out = dict(zip(self.PASSES, ms.tolist()))
        out['text_bytes'] = n.value
        out['out_bytes'] = m.value
        return out

    def close(self):
        if getattr(self, 'handle', None):
            _lib.lib().magot_tabcut_destroy(self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class SiteCounts(object):
    """composition_by_site's counting pass over a resident genome
    (magot_site_*, genome_tools.py:488-503): the alignment's rows are contigs of
    ``genome`` (``rows``: contig indices; default all of them, in order), each
    read from ``offsets`` (default 0) for ``n_sites`` sites (default: the
    first row's length from its offset).  Per site the rows holding a, t, c, g
    there in either case are counted; every other byte is left out.  A row
    shorter than its offset + n_sites is refused (MagotError)."""

    def __init__(self, genome, rows=None, offsets=None, n_sites=None):
        self.ctx = genome.ctx
        self.handle = None
        self._genome = genome  # the plane must outlive the handle
        rows = np.arange(len(genome.lengths)) if rows is None else np.asarray(rows).reshape(-1)
        rows = np.ascontiguousarray(rows, dtype=np.uint32)
        if offsets is None:
            offsets = np.zeros(len(rows), np.uint64)
        offsets = np.ascontiguousarray(np.asarray(offsets, dtype=np.uint64).reshape(-1))
        if len(offsets) != len(rows):
            raise ValueError('one offset per row')
        if n_sites is None and len(rows):
            n_sites = int(genome.lengths[int(rows[0])]) - int(offsets[0])
        self.n_rows, self.n_sites = len(rows), int(n_sites or 0)
        h = ctypes.c_void_p()
        check(_lib.lib().magot_site_create(self.ctx.handle, genome.handle, ptr(rows), ptr(offsets),
                                           self.n_rows, self.n_sites, ctypes.byref(h)),
              'magot_site_create')
        self.handle = h

    @staticmethod
    def _params():
        p = [ctypes.c_uint32() for _ in range(5)]
        _lib.lib().magot_site_params(*[ctypes.byref(x) for x in p])
        return [x.value for x in p]

    @staticmethod
    def sites_per_lane():
        """Consecutive sites one lane counts: one plane word of every row."""
        return SiteCounts._params()[0]

    @staticmethod
    def sites_per_tile():
        """Sites of one workgroup."""
        return SiteCounts._params()[1]

    @staticmethod
    def rows_per_strip():
        """Rows one workgroup goes down; an alignment with more is counted in
        strips whose counts are added with atomics."""
        return SiteCounts._params()[2]

    @staticmethod
    def widening_periods():
        """(rows after which the 4-bit counters are widened to bytes, rows after
        which the bytes are widened to 32 bits)."""
        return tuple(SiteCounts._params()[3:5])

    def counts(self):
        """n_sites x 4 uint32: the rows with a, t, c, g at each site."""
        check(_lib.lib().magot_site_execute(self.ctx.handle, self.handle), 'magot_site_execute')
        out = np.empty((self.n_sites, 4), np.uint32)
        check(_lib.lib().magot_site_counts(self.ctx.handle, self.handle, ptr(out)),
              'magot_site_counts')
        return out

    def time(self, iters):
        """Mean device ms of the counting pass (magot_site_time)."""
        ms = ctypes.c_double()
        check(_lib.lib().magot_site_time(self.ctx.handle, self.handle, int(iters), ctypes.byref(ms)),
              'magot_site_time')
        return ms.value

    def close(self):
        if getattr(self, 'handle', None):
            _lib.lib().magot_site_destroy(self.handle)
            self.handle = None
        self._genome = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def render_composition(counts, threads=0):
    """composition_by_site's text (a uint8 array) from n x 4 counts of a, t, c,
    g: the header line, then per site the four shares of their sum as Python
    2 prints a float (magot_site_render).  ZeroDivisionError, as the tool's, when
    a site has no counted base.  Host only."""
    counts = np.ascontiguousarray(np.asarray(counts, dtype=np.uint32))
    if counts.ndim != 2 or counts.shape[1] != 4:
        raise ValueError('counts must be n x 4')
    L = _lib.lib()
    text, n, empty = ctypes.c_void_p(), ctypes.c_uint64(), ctypes.c_uint64()
    rc = L.magot_site_render(ptr(counts) if len(counts) else None, len(counts), int(threads),
                             ctypes.byref(text), ctypes.byref(n), ctypes.byref(empty))
    if rc == _lib.ERR_RANGE:
        raise ZeroDivisionError('float division by zero (site %d)' % empty.value)
    check(rc, 'magot_site_render')
    try:
        return np.ctypeslib.as_array(ctypes.cast(text, ctypes.POINTER(ctypes.c_uint8)),
                                     shape=(n.value,)).copy()
    finally:
        L.magot_site_text_free(text)


class VariantHets(object):
    """heterozygosity_from_vcf's tables on the device (magot_vcf_*,
    magot_variants.py:16-139).  ``parse`` makes the VCF's text resident, indexes
    its lines and parses every data line, a wave each: POS, CPython 2.7's hash
    of ``CHROM<:>POS``, CHROM run heads, and per sample column one bit -- the
    column is the line's first field with its bytes (read_vcf's
    ``fields.index``) and its GT's first and last byte differ.  ``resolve``
    takes the contig of every CHROM run, keys the lines (contig, POS) and sorts
    them: a key's last line is kept.  ``count`` counts the kept lines' bits per
    locus, a range of the sorted keys.  ``parse`` returns (None, reason) outside
    the native grammar (_lib.VCF_REASONS).  Spans are (offset, length) into the
    text without the line's LF."""

    PASSES = ('line_index', 'classify', 'parse', 'runs', 'sort', 'flags', 'count', 'copy')

    def __init__(self):
        self.ctx = None
        self.handle = None
        self.n_lines = self.n_data = self.n_header = self.n_samples = self.words = self.n_runs = 0
        self.header = (0, 0)
        self.upload_ms = 0.0
        self.declined_line = 0

    @classmethod
    def parse(cls, data, max_bytes=0, max_samples=0, max_runs=0, ctx=None):
        """``max_bytes``: a longer text is declined (0: a quarter of the free
        device memory); ``max_samples``, ``max_runs``: lower limits than the
        device path's own, for tests."""
        self = cls()
        self.ctx = ctx or _lib.default_context()
        view = _text_view(data)
        h, reason, line = ctypes.c_void_p(), ctypes.c_uint32(), ctypes.c_uint64()
        rc = _lib.lib().magot_vcf_parse(self.ctx.handle, _text_ptr(view), len(view),
                                        int(max_bytes or 0), int(max_samples or 0),
                                        int(max_runs or 0), ctypes.byref(h), ctypes.byref(reason),
                                        ctypes.byref(line))
        if rc == _lib.ERR_UNSUPPORTED:
            VariantHets.last_declined_line = line.value
            return None, _lib.VCF_REASONS[reason.value]
        check(rc, 'magot_vcf_parse')
        self.handle = h
        n = [ctypes.c_uint64() for _ in range(3)]
        s, w = ctypes.c_uint32(), ctypes.c_uint32()
        r, ho, hl = ctypes.c_uint64(), ctypes.c_uint64(), ctypes.c_uint64()
        check(_lib.lib().magot_vcf_sizes(h, *[ctypes.byref(x) for x in n + [s, w, r, ho, hl]]),
              'magot_vcf_sizes')
        self.n_lines, self.n_data, self.n_header = [x.value for x in n]
        self.n_samples, self.words, self.n_runs = s.value, w.value, r.value
        self.header = (ho.value, hl.value)
        self.upload_ms = float(_lib.lib().magot_vcf_upload_ms(h))
        return self

    last_declined_line = 0  # 1-based line of the last decline (0: none named)

    @staticmethod
    def params():
        """(rows per piece of the counting pass, most samples, most CHROM runs,
        most counters)."""
        p = [ctypes.c_uint32() for _ in range(3)] + [ctypes.c_uint64()]
        _lib.lib().magot_vcf_params(*[ctypes.byref(x) for x in p])
        return tuple(x.value for x in p)

    def _spans(self, fn, name, n):
        off, length = np.zeros(max(n, 1), np.uint64), np.zeros(max(n, 1), np.uint64)
        check(fn(self.ctx.handle, self.handle, ptr(off), ptr(length)), name)
        return off[:n], length[:n]

    def header_lines(self):
        """The spans of the ``##`` lines in file order."""
        return self._spans(_lib.lib().magot_vcf_header_lines, 'magot_vcf_header_lines',
                           self.n_header)

    def runs(self):
        """The CHROM span of the first line of every run of data lines with one
        CHROM."""
        return self._spans(_lib.lib().magot_vcf_runs, 'magot_vcf_runs', self.n_runs)

    def resolve(self, contig_of_run):
        contig = np.ascontiguousarray(np.asarray(contig_of_run, dtype=np.uint32).reshape(-1))
        check(_lib.lib().magot_vcf_resolve(self.ctx.handle, self.handle, ptr(contig), len(contig)),
              'magot_vcf_resolve')

    def tables(self):
        """Per data line in file order, as a dict of arrays: 'line' (0-based),
        'pos', 'hash', 'kept', 'first' (the last and the first line of its key;
        zeros before ``resolve``) and 'bits' (n_data x words, uint32)."""
        n = max(self.n_data, 1)
        t = {'line': np.zeros(n, np.uint32), 'pos': np.zeros(n, np.int32),
             'hash': np.zeros(n, np.uint64), 'kept': np.zeros(n, np.uint8),
             'first': np.zeros(n, np.uint8), 'bits': np.zeros((n, max(self.words, 1)), np.uint32)}
        check(_lib.lib().magot_vcf_tables(self.ctx.handle, self.handle,
                                          *[ptr(t[k]) for k in ('line', 'pos', 'hash', 'kept',
                                                                'first', 'bits')]),
              'magot_vcf_tables')
        return {k: v[:self.n_data] for k, v in t.items()}

    def first_variant_line(self, order):
        """(line, off, len) of the line that holds ``list(variant_set)[0]``:
        the kept line of the first key as a Python 2 dict of the keys iterates
        (``order='py2'``, from the hashes) or of the first data line's key."""
        d = 0
        if order == 'py2':
            n = max(self.n_data, 1)
            hashes, first = np.zeros(n, np.uint64), np.zeros(n, np.uint8)
            check(_lib.lib().magot_vcf_tables(self.ctx.handle, self.handle, None, None,
                                              ptr(hashes), None, ptr(first), None),
                  'magot_vcf_tables')
            firsts = np.flatnonzero(first[:self.n_data])
            d = int(firsts[int(py2_order_of_hashes(hashes[firsts])[0])])
        line, off, length = ctypes.c_uint64(), ctypes.c_uint64(), ctypes.c_uint64()
        check(_lib.lib().magot_vcf_last_of(self.ctx.handle, self.handle, d, ctypes.byref(line),
                                           ctypes.byref(off), ctypes.byref(length)),
              'magot_vcf_last_of')
        return line.value, off.value, length.value

    def count(self, contig, lo, hi, allowed):
        """(counts, foreign): per locus -- the positions lo..hi of a contig,
        none when lo > hi -- and sample the kept lines inside with the sample's
        bit set (n_loci x n_samples, uint32); ``foreign``: one of those lines has
        a bit outside ``allowed`` (words x uint32).  (None, reason) above the
        most counters."""
        contig = np.ascontiguousarray(np.asarray(contig, dtype=np.uint32).reshape(-1))
        lo = np.ascontiguousarray(np.asarray(lo, dtype=np.uint32).reshape(-1))
        hi = np.ascontiguousarray(np.asarray(hi, dtype=np.uint32).reshape(-1))
        allowed = np.ascontiguousarray(np.asarray(allowed, dtype=np.uint32).reshape(-1))
        if not (len(contig) == len(lo) == len(hi)) or len(allowed) != self.words:
            raise ValueError('one contig, lo and hi per locus; one word per 32 samples')
        n = len(contig)
        counts = np.zeros((max(n, 1), self.n_samples), np.uint32)
        foreign, reason = ctypes.c_uint32(), ctypes.c_uint32()
        rc = _lib.lib().magot_vcf_count(self.ctx.handle, self.handle, ptr(contig), ptr(lo), ptr(hi),
                                        n, ptr(allowed), ptr(counts), ctypes.byref(foreign),
                                        ctypes.byref(reason))
        if rc == _lib.ERR_UNSUPPORTED:
            return None, _lib.VCF_REASONS[reason.value]
        check(rc, 'magot_vcf_count')
        return counts[:n], bool(foreign.value)

    def time(self, iters):
        """Mean device ms per pass (PASSES; 'count': the last ``count``'s loci,
        0 before one; 'copy': a device copy of the text, 'text_bytes' bytes)
        (magot_vcf_time)."""
        ms = np.zeros(len(self.PASSES), np.float64)
        n = ctypes.c_uint64()
        check(_lib.lib().magot_vcf_time(self.ctx.handle, self.handle, int(iters), ptr(ms),
                                        ctypes.byref(n)), 'magot_vcf_time')
        out = dict(zip(self.PASSES, ms.tolist()))
        out['text_bytes'] = n.value
        return out

    def close(self):
        if getattr(self, 'handle', None):
            _lib.lib().magot_vcf_destroy(self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def render_hets(loci, seqlen, counts, cols, threads=0):
    """calculate_heterozygosity's string from the het counts: per locus (a
    str) with seqlen >= 1 the locus and, for every column of ``cols``, 100.0 *
    count / seqlen as Python 2 prints a float; rows joined by LF
    (magot_vcf_render).  Host only."""
    counts = np.ascontiguousarray(np.asarray(counts, dtype=np.uint32))
    seqlen = np.ascontiguousarray(np.asarray(seqlen, dtype=np.int64).reshape(-1))
    cols = np.ascontiguousarray(np.asarray(cols, dtype=np.uint32).reshape(-1))
    n = len(loci)
    if counts.ndim != 2 or len(counts) != n or len(seqlen) != n:
        raise ValueError('one row of counts and one length per locus')
    parts = [s.encode('latin-1') for s in loci]
    off = np.zeros(n + 1, np.uint64)
    if n:
        off[1:] = np.cumsum(np.fromiter((len(b) for b in parts), np.uint64, n))
    blob = b''.join(parts)
    L = _lib.lib()
    text, size = ctypes.c_void_p(), ctypes.c_uint64()
    check(L.magot_vcf_render(blob, ptr(off), ptr(seqlen) if n else None,
                             ptr(counts) if counts.size else None, n, counts.shape[1],
                             ptr(cols) if len(cols) else None, len(cols), int(threads),
                             ctypes.byref(text), ctypes.byref(size)), 'magot_vcf_render')
    try:
        return ctypes.string_at(text, size.value).decode('latin-1')
    finally:
        L.magot_site_text_free(text)


def copy_segments(src_dev_ptr, src_bytes, dst_dev_ptr, src_off, dst_off, ctx=None):
    """dst[dst_off[i]:dst_off[i+1]] = src[src_off[i]:...] on the device
    (magot_copy_segments; addresses of device memory, src_bytes the source's
    size, host offset tables)."""
    ctx = ctx or _lib.default_context()
    so = np.ascontiguousarray(src_off, dtype=np.uint64)
    do = np.ascontiguousarray(dst_off, dtype=np.uint64)
    if len(do) != len(so) + 1:
        raise ValueError('dst_off needs len(src_off) + 1 entries')
    check(_lib.lib().magot_copy_segments(ctx.handle, ctypes.c_void_p(src_dev_ptr), int(src_bytes),
                                         ctypes.c_void_p(dst_dev_ptr), ptr(so), ptr(do), len(so)),
          'magot_copy_segments')


def orf6_sizes(rec_off):
    """(stream_off 6n+1, stream_len 6n) of the six-frame layout over records
    with nucleotide offsets ``rec_off`` (n+1): magot_orf6_sizes."""
    off = np.ascontiguousarray(rec_off, dtype=np.uint64)
    n = len(off) - 1
    soff = np.empty(6 * n + 1, dtype=np.uint64)
    slen = np.empty(max(6 * n, 1), dtype=np.uint64)
    check(_lib.lib().magot_orf6_sizes(ptr(off), n, ptr(soff), ptr(slen), None), 'magot_orf6_sizes')
    return soff, slen[:6 * n]


def codon_symbols(seq, class256, n_classes, lut, ctx=None):
    """One symbol per full codon of ``seq`` (str/bytes, length a multiple of 3)
    over an extended alphabet (magot_codon_symbols): a list of ints."""
    ctx = ctx or _lib.default_context()
    buf = np.frombuffer(_as_bytes(seq), dtype=np.uint8)
    m = len(buf) // 3
    out = np.empty(max(m, 1), dtype=np.uint8)
    cls = np.ascontiguousarray(class256, dtype=np.uint8)
    lt = np.ascontiguousarray(lut, dtype=np.uint8)
    check(_lib.lib().magot_codon_symbols(ctx.handle, ptr(buf) if m else None, m, ptr(cls),
                                         int(n_classes), ptr(lt), ptr(out)),
          'magot_codon_symbols')
    return out[:m].tolist()


def translate_batch(seqs, frames, strands, lut64=None, ctx=None):
    """Untrimmed Sequence.translate (genome.py:795-822) residues per input, or None
    where the reference returns None.  The caller applies trimX."""
    ctx = ctx or _lib.default_context()
    n = len(seqs)
    buf, off = _concat(seqs)
    fr = np.ascontiguousarray(frames, dtype=np.int32)
    st = np.frombuffer(''.join(strands).encode('latin-1'), dtype=np.uint8).copy() if n else \
        np.zeros(0, np.uint8)
    poff = np.empty(n + 1, dtype=np.uint64)
    codons = np.empty(max(n, 1), dtype=np.int64)
    L = _lib.lib()
    check(L.magot_translate_sizes(ptr(off), n, ptr(fr), ptr(poff), ptr(codons)),
          'magot_translate_sizes')
    total = int(poff[n])
    out = np.empty(max(total, 1), dtype=np.uint8)
    lut = None
    if lut64 is not None:
        lut = np.frombuffer(bytes(lut64), dtype=np.uint8).copy()
    check(L.magot_translate_batch(ctx.handle, ptr(buf) if len(buf) else None, ptr(off), n,
                                  ptr(fr), ptr(st), ptr(lut), ptr(poff), ptr(out)),
          'magot_translate_batch')
    raw = out.tobytes()
    res = []
    for i in range(n):
        if codons[i] < 0:
            res.append(None)
        else:
            res.append(raw[int(poff[i]):int(poff[i + 1])].decode('latin-1'))
    return res


__all__ = ['DeviceGenome', 'ExtractionPlan', 'revcomp_batch', 'translate_batch', 'codon_symbols',
           'OUT_NUC',
           'OUT_PEP', 'MagotError', 'GffPlan', 'orf6_batch', 'Orf6Plan', 'fasta_read',
           'FastaGenome', 'PartitionedGenome', 'device_genome', 'extract_records', 'plan_parts',
           'copy_segments', 'orf6_sizes', 'OrfCalls', 'ORFCALL_TILE', 'ORF_TABLE_DTYPE',
           'LongestOrfs', 'LONGORF_TABLE_DTYPE', 'CdsPlan',
           'GenomeTrack', 'TrackWindows', 'interval_pieces', 'ReadLengths']
