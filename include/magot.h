/*
 * magot.h -- C ABI of libmagot.so, the MI355X (gfx950) extraction engine behind
 * the magot_amd Python package.
 *
 * The reference (Huangtianyu-caas/MAGOT, Python 2.7) has no FFI: its hot path is
 * the pure-Python call chain
 *     AnnotationSet.get_fasta          genome.py:578-582
 *       ParentAnnotation.get_fasta     genome.py:677-731
 *         BaseAnnotation.get_seq       genome.py:603-614
 *           Sequence.reverse_compliment genome.py:784-793
 *         Sequence.translate           genome.py:795-822
 * over a GenomeSequence dict (genome.py:854-877).  This header is the boundary
 * that chain is cut at: the Python layer (magot_amd/genome.py) walks the
 * annotation graph exactly as the reference does and hands the resulting
 * interval lists to this library; every byte of sequence output is produced
 * by HIP kernels.  Plain pointers and sizes only -- no torch types.
 *
 * Ownership: callers own every host buffer; the library owns device memory
 * behind the opaque handles, released by the matching *_destroy.
 * Errors: every int-returning call returns MAGOT_OK (0) or a negative status;
 * magot_last_error() gives a thread-local message.
 * Threading: a magot_ctx is bound to one device and one HIP stream and is not
 * thread-safe; use one context per host thread.  One process per GPU.
 */
#ifndef MAGOT_H
#define MAGOT_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MAGOT_ABI_VERSION 1

enum magot_status {
  MAGOT_OK = 0,
  MAGOT_ERR_ARG = -1,      /* bad argument / inconsistent tables           */
  MAGOT_ERR_HIP = -2,      /* HIP runtime failure (no device, OOM, fault)   */
  MAGOT_ERR_RANGE = -3,    /* interval outside its contig                   */
  MAGOT_ERR_STATE = -4,    /* call out of order (e.g. fetch before execute) */
  MAGOT_ERR_UNSUPPORTED = -5 /* input takes a reference diagnostic path: use the
                                Python object path (magot_gff_plan)              */
};

/* Output selection for a plan (magot_plan_create.outputs). */
#define MAGOT_OUT_NUC 1u   /* spliced CDS nucleotides  (seq_type="nucleotide") */
#define MAGOT_OUT_PEP 2u   /* frame-0 translation      (seq_type="protein")    */
/* Layout flag: lay the records out in the device buffers in genome order (by
 * the coordinate of each record's first non-empty interval) instead of record
 * order.  Neighbouring loci then run in neighbouring tiles and share genome
 * lines.  magot_plan_fetch, magot_plan_copy_outputs and magot_fasta_text_*
 * still deliver record order (a device segment copy puts the records back);
 * magot_plan_layout gives each record's place in the device buffers.  Such a
 * plan has no six-frame plan (magot_plan_orf6 refuses it). */
#define MAGOT_OUT_GENOME_ORDER 4u

/*
 * One interval of one record, already in OUTPUT order.
 *   start_rc : bits 0..62 = 0-based start inside the contig (the Python slice
 *              contig[c0-1:c1] already normalised by slice.indices, so
 *              genome.py:606/608 semantics incl. clamping are resolved);
 *              bit 63 = reverse-complement this interval (strand '-',
 *              genome.py:607-608).
 *   contig   : index into the contig list given to magot_genome_load.
 *   len      : number of bases (0 allowed: empty Python slice).
 * Replaces: BaseAnnotation.get_seq (genome.py:603-614) per child, ordered as
 * ParentAnnotation.get_fasta orders them (genome.py:689-703).
 */
typedef struct magot_exon {
  uint64_t start_rc;
  uint32_t contig;
  uint32_t len;
} magot_exon;

/*
 * One output record = the contiguous exon range [exon_begin, exon_begin+n_exons).
 * Records must tile the exon table in order (exon_begin[t+1] ==
 * exon_begin[t] + n_exons[t]).  flags is reserved (0).
 * Replaces: the "".join of genome.py:702-705 for one ParentAnnotation.
 */
typedef struct magot_tx {
  uint64_t exon_begin;
  uint32_t n_exons;
  uint32_t flags;
} magot_tx;

typedef struct magot_ctx magot_ctx;
typedef struct magot_genome magot_genome;
typedef struct magot_plan magot_plan;

/* ABI version compiled into the library (== MAGOT_ABI_VERSION). */
int magot_abi_version(void);

/* Thread-local text of the last failure on this thread ("" if none). */
const char* magot_last_error(void);

/* Number of visible HIP devices (0 when none / runtime unavailable). */
int magot_device_count(void);

/* Bind a context to HIP device `device` with a private non-blocking stream. */
int magot_ctx_create(int device, magot_ctx** out);
void magot_ctx_destroy(magot_ctx* ctx);

/*
 * Pack a genome into HBM: a nibble plane (2-bit ACGT code, soft-mask bit,
 * exception bit per base) plus its reverse-complement mirror, and a run list
 * of every byte that is not ACGTacgt (N, IUPAC, '-', spaces ...) with a
 * 4096-base directory.  seqs[i] points at lens[i] raw bytes of contig i,
 * exactly the bytes genome.py:875 keeps (every byte except CR/LF).  One
 * device plane holds up to ~4 Gbases; above that MAGOT_ERR_UNSUPPORTED, and
 * the caller packs the contigs as several planes, one magot_genome each
 * (magot_amd.engine.PartitionedGenome: one plan per plane).
 * Replaces: GenomeSequence (genome.py:854-877) as the data the path reads.
 */
int magot_genome_load(magot_ctx* ctx, const uint8_t* const* seqs, const uint64_t* lens,
                      uint32_t n_contigs, magot_genome** out);
/*
 * The same with flags.  By default (and in magot_genome_load /
 * magot_genome_load_fasta) the packing runs on the device: the raw bytes are
 * streamed into HBM once through pinned buffers and kernels build the nibble
 * plane, its mirror and the exception runs (the run list's directory is built
 * on the host from the runs).  MAGOT_PACK_HOST packs on the host (pack.cpp,
 * the sanitizer-tested twin) and uploads the plane; both give the same arena
 * bytes (tests/test_gpu_replication.py).
 */
#define MAGOT_PACK_HOST 1u
int magot_genome_load_ex(magot_ctx* ctx, const uint8_t* const* seqs, const uint64_t* lens,
                         uint32_t n_contigs, uint32_t flags, magot_genome** out);
/*
 * Read FASTA text (GenomeSequence, genome.py:854-877, incl. truncate_names)
 * natively and pack it like magot_genome_load (MAGOT_ERR_UNSUPPORTED above
 * one device plane, as there).  MAGOT_ERR_UNSUPPORTED also for
 * headers whose whitespace split differs between the reference's Python 2
 * byte strings and Python 3 (bytes >= 0x80, 0x1c-0x1f) or that are empty
 * under truncate_names: the caller then uses the Python reader.
 * magot_genome_contigs: contig count, lengths and NUL-separated names (names
 * only for genomes read by magot_genome_load_fasta; NULL buffers = sizes).
 */
int magot_genome_load_fasta(magot_ctx* ctx, const char* text, uint64_t len, int truncate_names,
                            magot_genome** out);
int magot_genome_contigs(const magot_genome* g, uint32_t* n, uint64_t* lens, char* names,
                         uint64_t names_cap, uint64_t* names_len);
/* Host-only: the same FASTA reader into caller buffers (first call with NULL
 * buffers for the count, lengths and name bytes; lens needs n entries). */
int magot_fasta_read(const char* text, uint64_t len, int truncate_names, uint32_t* n,
                     uint64_t* lens, char* names, uint64_t names_cap, uint64_t* names_len,
                     uint8_t* seqs, uint64_t seqs_cap);

/*
 * cds2pep (genome_tools.py:664-675) without a per-line loop.  magot_cds_scan
 * splits `text` into lines ('\n'; a CR before it is dropped): lines starting
 * with '>' are headers (hdr_off / hdr_len[n_seg-1]), all others are appended
 * to the current sequence; segment k (seq[seg_off[k]:seg_off[k+1]], n_seg+1
 * offsets) is the sequence before header k, the last one follows the last
 * header.  Call with NULL buffers for n_seg / seq_bytes first.
 * MAGOT_ERR_UNSUPPORTED: an empty line (the reference's IndexError) or a CR
 * inside a line; the caller's line loop reproduces both.  magot_cds_render
 * writes the tool's stdout from the frame-0 translations of the segments
 * (magot_translate_batch layout: poff, codons < 0 for None): a translation
 * for every non-empty segment before a header and for the last one ("None"
 * when translate() returns None, one leading 'X' trimmed), each header after
 * its segment.  out == NULL: *out_len only.
 */
int magot_cds_scan(const char* text, uint64_t len, uint64_t* n_seg, uint64_t* seq_bytes,
                   uint64_t* seg_off, uint64_t* hdr_off, uint64_t* hdr_len, uint8_t* seq,
                   uint64_t seq_cap);
int magot_cds_render(const char* text, uint64_t n_seg, const uint64_t* seg_off,
                     const uint64_t* hdr_off, const uint64_t* hdr_len, const uint8_t* pep,
                     const uint64_t* poff, const int64_t* codons, uint8_t* out, uint64_t cap,
                     uint64_t* out_len);

/* Sizes of a loaded genome: total bases, exception runs, device bytes held. */
int magot_genome_stats(const magot_genome* g, uint64_t* total_bases, uint64_t* n_exc_runs,
                       uint64_t* device_bytes);
void magot_genome_destroy(magot_genome* g);

/*
 * Genome replication across ranks (one packed genome broadcast
 * over RCCL/xGMI instead of every rank packing its own).  The packed genome
 * is one device arena plus a host meta blob:
 *   magot_genome_export    meta blob (meta == NULL: size only) and arena size;
 *   magot_genome_copy_arena D2D copy of the arena into caller device memory
 *                          (e.g. the tensor a collective broadcasts);
 *   magot_genome_attach    a genome over caller device memory holding a
 *                          broadcast arena (not freed by magot_genome_destroy).
 */
int magot_genome_export(const magot_genome* g, uint8_t* meta, uint64_t cap, uint64_t* meta_len,
                        uint64_t* arena_bytes);
int magot_genome_copy_arena(const magot_genome* g, void* dst_dev);
int magot_genome_attach(magot_ctx* ctx, const uint8_t* meta, uint64_t meta_len, void* arena_dev,
                        magot_genome** out);
/*
 * What a replica must receive: magot_genome_wire_ranges gives the *n (= 2)
 * byte ranges [off[k], off[k]+len[k]) of the arena to transfer -- the forward
 * nibble plane (span/2 bytes), then the exception runs and their directory.
 * The reverse-strand mirror between them (as many bytes again) is a pure
 * function of the forward plane (genome.py:784-793), so
 * magot_genome_attach_wire attaches like magot_genome_attach and then rebuilds
 * the mirror on the receiving device: half the bytes cross xGMI.  The caller
 * memory must be arena_bytes long and hold the wire ranges at their offsets.
 */
int magot_genome_wire_ranges(const magot_genome* g, uint64_t* off, uint64_t* len, uint32_t* n);
int magot_genome_attach_wire(magot_ctx* ctx, const uint8_t* meta, uint64_t meta_len,
                             void* arena_dev, magot_genome** out);
/*
 * The compact replica image (what a multi-GPU job broadcasts; the north
 * star's 2-bit-packed genome): the forward strand's 2-bit codes (span/4
 * bytes), the soft-masked bases as sorted {start, end} u32 runs plus a
 * directory of one u32 per 4096 bases, and the arena's exception runs +
 * directory verbatim -- every GenomeSequence byte (genome.py:854-877), about
 * 0.27 B per base against the arena's 1 B.
 *   magot_genome_wire_export  writes the image of g into caller device memory
 *       of cap bytes (wire_dev == NULL: *wire_bytes only).  Synchronous.
 *   magot_genome_wire_import  a genome in its own new arena (freed by
 *       magot_genome_destroy) rebuilt on ctx's device from an image in device
 *       memory and the genome's meta blob (magot_genome_export): the nibble
 *       plane is unpacked and the mirror derived there; the arena equals the
 *       packed original byte for byte.  The image may be freed on return.
 *       An image that does not match the meta is refused (MAGOT_ERR_ARG).
 * No reference counterpart (the reference is single-process).
 */
int magot_genome_wire_export(const magot_genome* g, void* wire_dev, uint64_t cap,
                             uint64_t* wire_bytes);
int magot_genome_wire_import(magot_ctx* ctx, const uint8_t* meta, uint64_t meta_len,
                             const void* wire_dev, uint64_t wire_bytes, magot_genome** out);

/*
 * Reassembly of a sharded job's outputs on one device (outputs
 * gathered back, final order restored from the global record index): for
 * i < n, dst[dst_off[i], dst_off[i+1]) = src[src_off[i], src_off[i] +
 * dst_off[i+1] - dst_off[i]).  src (src_bytes long) and dst (dst_off[n] long)
 * are device memory (e.g. the buffer an RCCL gather filled, rank-major),
 * both 16-byte aligned (else MAGOT_ERR_ARG),
 * dst_off has n+1 non-decreasing entries, the offset tables are host arrays;
 * a segment reaching past src_bytes is refused (MAGOT_ERR_RANGE) before any
 * launch, and so is a segment of 4 GiB or more (MAGOT_ERR_ARG: the grouped
 * copy counts 16-byte chunks in 32 bits; split such a segment).  Synchronous.
 * No reference counterpart (the reference is single-process).
 */
int magot_copy_segments(magot_ctx* ctx, const void* src_dev, uint64_t src_bytes, void* dst_dev,
                        const uint64_t* src_off, const uint64_t* dst_off, uint64_t n);

/*
 * Build a device-resident plan: interval table -> output offsets, ~3 KiB
 * wave tiles, per-tile exon and record ranges, all uploaded to HBM.
 * nuc_bytes / pep_bytes receive the total output sizes (pep_bytes counts the
 * untrimmed frame-0 translation, floor(len/3) per record; the single leading
 * 'X' trim of genome.py:819-821 is applied by the caller on fetch).
 */
int magot_plan_create(magot_ctx* ctx, const magot_genome* g, const magot_exon* exons,
                      uint64_t n_exons, const magot_tx* txs, uint64_t n_tx, uint32_t outputs,
                      magot_plan** out, uint64_t* nuc_bytes, uint64_t* pep_bytes);
void magot_plan_destroy(magot_plan* p);

/* Enqueue the fused gather + reverse-complement + translate kernel on the
 * context stream (asynchronous; outputs stay in HBM). */
int magot_plan_execute(magot_ctx* ctx, magot_plan* p);

/* Block until the context stream is idle. */
int magot_ctx_sync(magot_ctx* ctx);

/* Timing marks on the context stream: magot_ctx_mark(ctx, 0) and (ctx, 1)
 * record events before and after a region of enqueued work (e.g. bench.py's
 * K timed steps); magot_ctx_elapsed waits for mark 1 and gives the GPU time
 * between them in ms.  No reference counterpart (measurement). */
int magot_ctx_mark(magot_ctx* ctx, int which);
int magot_ctx_elapsed(magot_ctx* ctx, double* ms);

/* Device facts of a context: compute units, and the extraction kernel's
 * resident workgroups per CU as launched (its occupancy cap included).  Any
 * pointer may be NULL.  No reference counterpart (diagnostics for bench.py). */
int magot_ctx_info(const magot_ctx* ctx, int* n_cu, int* extract_blocks_per_cu);

/* Copy outputs to caller buffers (synchronous).  Any pointer may be NULL to
 * skip it.  nuc_off / pep_off receive n_tx+1 prefix offsets.  A plan built
 * with MAGOT_OUT_GENOME_ORDER is put back into record order on the device on
 * the way down, through a transient device scratch of at most 256 MiB (or
 * the longest record, if longer) plus 16 bytes, batch by batch of records. */
int magot_plan_fetch(magot_ctx* ctx, magot_plan* p, uint8_t* nuc_out, uint64_t* nuc_off,
                     uint8_t* pep_out, uint64_t* pep_off);

/* execute + sync + fetch. */
int magot_run(magot_ctx* ctx, magot_plan* p, uint8_t* nuc_out, uint64_t* nuc_off,
              uint8_t* pep_out, uint64_t* pep_off);

/*
 * Kernel timing: execute `iters` times back to back on the context stream with
 * HIP events around each launch; *avg_ms receives the mean launch duration.
 */
int magot_plan_time(magot_ctx* ctx, magot_plan* p, int iters, double* avg_ms);
/* The same with ONE event pair around `iters` back-to-back launches: the
 * per-launch time of a step loop, the figure bench.py's roofline uses (it
 * agrees with rocprofv3's kernel-trace average; an isolated launch also pays
 * the launch latency, which dominates small plans such as C2). */
int magot_plan_time_b2b(magot_ctx* ctx, magot_plan* p, int iters, double* avg_ms);

/* D2D copy of a plan's outputs (nuc_bytes / pep_bytes) into caller device
 * memory, e.g. the buffers an output gather sends, in record order (a
 * genome-ordered plan's records are put back by a segment copy: its
 * destinations must then be 16-byte aligned, else MAGOT_ERR_ARG). */
int magot_plan_copy_outputs(magot_ctx* ctx, magot_plan* p, void* nuc_dst_dev, void* pep_dst_dev);

/* Device-resident output pointers of a plan (for on-device consumers/tests).
 * The buffers hold the records in the plan's layout order: record t starts at
 * magot_plan_layout's nuc_start[t] / pep_start[t] and is as long as its
 * prefix offsets (magot_plan_fetch) say. */
int magot_plan_device_outputs(magot_plan* p, void** nuc_dev, void** pep_dev);

/* Each record's start in the plan's device buffers (n_tx entries each; either
 * pointer may be NULL): the prefix offsets for a record-order plan, the
 * genome-order places for a MAGOT_OUT_GENOME_ORDER one.  No reference
 * counterpart (device layout). */
int magot_plan_layout(const magot_plan* p, uint64_t* nuc_start, uint64_t* pep_start);

/* Algorithmic byte count per execute of a plan (the roofline numerator):
 * ceil(B/4) + B*[nuc] + P*[pep] + 16*E + 32*T. */
uint64_t magot_plan_algorithmic_bytes(const magot_plan* p);

/* Debug (no device): the packed per-tile descriptor blocks magot_plan_create
 * uploads, from the planner's u64 tables.  ex_g / ex_out / tx_nuc / tx_pep as
 * the planner builds them (interval start | flag bits 63..61, n+1 output
 * offsets, record output / residue starts with their sentinel); tiles =
 * n_tiles rows {u64 T0, T1, Q0, Q1; u32 e1, e2, j1, j2}; lane_chunks 3 or 6.
 * geometry[3]: in, the inline interval / record rows of a block to force (0:
 * the planner's choice for these tiles); out, the rows used and the block
 * stride in bytes.  blocks receives stride bytes per tile, ovf_ex / ovf_tx
 * the overflow rows (8 / 16 bytes each); n_ovf[0..1] their counts.
 * blocks == NULL: geometry and counts only. */
int magot_debug_tile_blocks(const uint64_t* ex_g, const uint64_t* ex_out, const uint64_t* tx_nuc,
                            const uint64_t* tx_pep, uint64_t span, uint32_t lane_chunks,
                            const void* tiles, uint64_t n_tiles, uint32_t* geometry, void* blocks,
                            uint64_t* ovf_ex, uint64_t ovf_ex_cap, int64_t* ovf_tx,
                            uint64_t ovf_tx_cap, uint64_t* n_ovf);

/* Debug (no device): magot_plan_create's tile cut over the planner's tables,
 * in output order.  ex_out = n_ex + 1 output offsets of the non-empty
 * intervals; tx_nuc / tx_pep = output / residue starts of the n_rec records
 * with a codon, then their sentinel (output bytes, residues); lane_chunks 3
 * or 6.  tiles receives *n_tiles rows as in magot_debug_tile_blocks (at most
 * tiles_cap).  tiles == NULL: the count only. */
int magot_debug_tile_cut(const uint64_t* ex_out, uint64_t n_ex, const uint64_t* tx_nuc,
                         const uint64_t* tx_pep, uint64_t n_rec, uint32_t lane_chunks, void* tiles,
                         uint64_t tiles_cap, uint64_t* n_tiles);

/* Debug (no device): the six-frame kernel's tile cut (orf6_plan_tiles), as
 * magot_orf6_batch and magot_plan_orf6 upload it.  noff = n_rec + 1 offsets of
 * the records in the walked concatenation.  row_start = the n_rows starts of
 * the non-empty intervals in it, ascending, then noff[n_rec] as their sentinel
 * (n_rows + 1 entries), or NULL for the raw-byte batch, which has no interval
 * rows.  t0 receives *n_tiles + 1 tile starts (the last one the total), r0
 * the record holding each start; e0 (the interval holding each staged
 * window's first base) and m (the window's rows, capped) are written only
 * with row_start and may be NULL without it.  At most tiles_cap tiles are
 * written; t0 == NULL: the count only. */
int magot_debug_orf6_tiles(const uint64_t* noff, uint64_t n_rec, const uint64_t* row_start,
                           uint64_t n_rows, uint64_t* t0, uint32_t* r0, uint32_t* e0, uint32_t* m,
                           uint64_t tiles_cap, uint64_t* n_tiles);

/* Debug (no device): everything magot_plan_create plans before it touches
 * the device, for contigs given as to magot_genome_load (packed on the host)
 * and tables and output flags given as to magot_plan_create; the same status
 * and magot_last_error text on a bad table.  The MAGOT_EXTRACT_LANE_CHUNKS
 * and MAGOT_TILE_BLOCK_ROWS overrides apply as they do there.
 * info[9] = output bytes, residues, non-empty intervals Ec, records with a
 * codon Tc, tiles, lane chunks, inline interval rows, inline record rows,
 * block stride.  tiles == NULL: info only.  Otherwise info must hold what
 * that first call gave, and ex_g / ex_out receive Ec + 1 rows (interval start
 * | flag bits 63..61, output offset; layout order), tx_nuc / tx_pep Tc + 1,
 * lay_nuc / lay_pep each record's place in the layout (n_tx), tiles the tiles
 * in launch order. */
int magot_debug_plan(const uint8_t* const* seqs, const uint64_t* lens, uint32_t n_contigs,
                     const magot_exon* exons, uint64_t n_exons, const magot_tx* txs, uint64_t n_tx,
                     uint32_t outputs, uint64_t* info, uint64_t* ex_g, uint64_t* ex_out,
                     uint64_t* tx_nuc, uint64_t* tx_pep, uint64_t* lay_nuc, uint64_t* lay_pep,
                     void* tiles);

/* Debug: the byte index that magot_psl_parse, magot_vcf_parse,
 * magot_fastarec_parse and magot_rename_parse begin with, on its own.  The
 * len bytes of text go to the device; the first index_len <= len of them are
 * the text that is indexed (the rest lie behind its end and must not be
 * counted).  *n_out: the occurrences of `byte` (0..255) in it; pos_out (NULL,
 * or room for index_len entries) receives their offsets in text order;
 * *second_count_out (may be NULL) the occurrences of second_byte, -1 for none. */
int magot_debug_text_index(magot_ctx* ctx, const uint8_t* text, uint64_t len, uint64_t index_len,
                           uint32_t byte, int32_t second_byte, uint64_t* pos_out, uint64_t* n_out,
                           uint64_t* second_count_out);

/* Debug: the same index in line mode, as the four tools run it: the count of
 * LF, then the fill of the line starts, with the stray-CR check when check_cr
 * is not 0.  len and index_len as above.  *n_lines_out: the LFs of the text,
 * and one more when it does not end in LF; pos_out (NULL, or room for
 * index_len + 2 entries) receives n_lines + 1 line starts, pos[0] = 0 and
 * pos[n_lines] = index_len; nothing is filled or written when n_lines is 0.
 * *stray_out (may be NULL) receives the raw status word, the lowest
 * line << 8 | stray_reason (0..255) over the CRs that are neither before an LF
 * nor the text's last byte, or all ones when there is none (always, without
 * check_cr). */
int magot_debug_text_lines(magot_ctx* ctx, const uint8_t* text, uint64_t len, uint64_t index_len,
                           int check_cr, uint32_t stray_reason, uint64_t* pos_out,
                           uint64_t* n_lines_out, uint64_t* stray_out);

/* Debug: the grouped piece copy of the FASTA reflow and the renamed text on
 * its own: piece i is the len[i] bytes at base + src[i], copied to
 * out + dst[i], 16 consecutive pieces per wave.  base (base_len bytes) goes
 * to the device with the padding the copy asks for; out (out_len bytes) is
 * uploaded, written by the copy and copied back whole, so every byte no piece
 * covers comes back as the caller's.  A piece outside base or out is
 * MAGOT_ERR_RANGE before any launch (out is then untouched); base_len and
 * out_len are below 2^28 (MAGOT_ERR_ARG).  Destinations must not overlap. */
int magot_debug_piece_copy(magot_ctx* ctx, const uint8_t* base, uint64_t base_len,
                           const uint64_t* src, const uint64_t* dst, const uint32_t* len,
                           uint64_t n, uint8_t* out, uint64_t out_len);

/* Debug: the FASTA text assembly of magot_fasta_text_execute on its own, over
 * tables of the caller's.  Unit i is text[text_off, text_off + text_len)
 * followed by the payload of record rec, pay[rspan[2 rec], rspan[2 rec + 1]),
 * or by nothing (rec = MAGOT_NO_RECORD); with protein not 0 a payload that
 * begins with 'X' loses that byte.  The units are written one behind the
 * other from out[0]; out (out_len bytes) is uploaded and copied back whole as
 * in magot_debug_piece_copy, and *written is the text's length.  A unit or a
 * record span outside its buffer, a rec >= n_rec and a text longer than
 * out_len are MAGOT_ERR_RANGE before any launch; text_len, pay_len and
 * out_len are below 2^28 (MAGOT_ERR_ARG). */
#define MAGOT_NO_RECORD 0xFFFFFFFFu
typedef struct magot_text_unit {
  uint64_t text_off;
  uint32_t text_len;
  uint32_t rec;
} magot_text_unit;
int magot_debug_text_assembly(magot_ctx* ctx, const magot_text_unit* units, uint64_t n,
                              const uint8_t* text, uint64_t text_len, const uint64_t* rspan,
                              uint64_t n_rec, const uint8_t* pay, uint64_t pay_len, int protein,
                              uint8_t* out, uint64_t out_len, uint64_t* written);

/*
 * Raw-sequence batch ops over n byte strings (seq_off has n+1 entries).
 * Replaces: Sequence.reverse_compliment (genome.py:784-793).
 * out must hold seq_off[n] bytes; record i lands at out[seq_off[i]...].
 */
int magot_revcomp_batch(magot_ctx* ctx, const uint8_t* seqs, const uint64_t* seq_off, uint64_t n,
                        uint8_t* out);

/*
 * Replaces: Sequence.translate (genome.py:795-822) for frame >= 0, strand
 * '+'/'-'.  codons_out[i] = number of emitted residues (before trimX), or -1
 * when the reference returns None (len <= 2 + frame).  pep_off (n+1) must be
 * filled by magot_translate_sizes first; out holds pep_off[n] bytes.
 * magot_translate_batch refuses (MAGOT_ERR_ARG, before it touches the device)
 * a seq_off that is not non-decreasing, a negative frame, and a pep_off that
 * is not magot_translate_sizes' table for seq_off and frames.
 * lut64 maps codon c0 + 4*c1 + 16*c2 (A=0,C=1,G=2,T=3) to a residue byte;
 * NULL = the standard code of genome.py:795-802.  The junk first codon of
 * frames 1/2 (genome.py:811-818) is emitted as 'X'.
 */
int magot_translate_sizes(const uint64_t* seq_off, uint64_t n, const int32_t* frames,
                          uint64_t* pep_off, int64_t* codons_out);
int magot_translate_batch(magot_ctx* ctx, const uint8_t* seqs, const uint64_t* seq_off, uint64_t n,
                          const int32_t* frames, const uint8_t* strands, const uint8_t* lut64,
                          const uint64_t* pep_off, uint8_t* out);

/*
 * Single-sequence forms of the two (the SURVEY 8(b) sketch), same semantics.
 * magot_revcomp: out holds len bytes.  magot_translate: standard code, frame
 * >= 0 (MAGOT_ERR_UNSUPPORTED below: the Python layer lays negative frames out
 * itself), strand '+' or '-', trimX 0/1; out must hold (len + 2) / 3 bytes
 * (frames 1 and 2 emit a junk first codon: frame 1 of a length with len % 3
 * == 2 gives (len + 1) / 3 residues before the trim); exactly *out_len bytes
 * are written; *out_len = residues, or -1 where the reference returns None.
 */
int magot_revcomp(magot_ctx* ctx, const uint8_t* seq, uint64_t len, uint8_t* out);
int magot_translate(magot_ctx* ctx, const uint8_t* seq, uint64_t len, int frame, int strand,
                    int trimX, uint8_t* out, int64_t* out_len);

/*
 * Sequence.translate with an arbitrary codon `library` (genome.py:795-818:
 * any dict -- keys that are not ACGT triplets, e.g. 'NNN', multi-character
 * values -- and any integer frame, negative included).  The caller lays out
 * the characters the reference's loop visits and drops the first (junk)
 * codon; this computes one symbol per full codon of seq[0, 3*n_codons):
 * out[k] = lut[c0 + K*c1 + K*K*c2], c = class256[byte] (upper-case folding
 * and the library's key characters folded into K = n_classes classes,
 * K^3 <= 32768).  The caller maps symbols to the library's values.
 */
int magot_codon_symbols(magot_ctx* ctx, const uint8_t* seq, uint64_t n_codons,
                        const uint8_t* class256, uint32_t n_classes, const uint8_t* lut,
                        uint8_t* out);

/*
 * Six-frame translation for Sequence.get_orfs (genome.py:824-851): for each
 * record, translate(frame=f, strand) for f = 0,1,2 and strand '-','+' in the
 * reference's loop order.  Stream j = 6*record + 2*f + (strand == '+') holds
 * the REAL codons only: frames 1/2 start with a junk 1-/2-base codon that
 * trimX always drops (genome.py:809-821), so it is not emitted; frame 0 is
 * untrimmed (the caller drops one leading 'X').  Streams start on 16-byte
 * boundaries, a record's three '-' streams before its three '+' streams
 * (strand-major: the kernel writes each strand's chunks in one pass):
 * stream_off (6n+1) are the padded offsets (stream_off[6n] the total),
 * stream_len (6n) the real residue counts, and the padding bytes are 0;
 * none_mask[j] = 1 where the reference returns None (len <= 2 + f).  Because
 * of the strand-major placement stream_off[j+1] is NOT where stream j's
 * padding ends: stream j occupies [stream_off[j], stream_off[j] +
 * pad16(stream_len[j])), pad16(x) = (x + 15) & ~15, and a record's six streams
 * are one contiguous block [stream_off[6r], stream_off[6r+6]).  Callers that
 * need the extents must pass stream_len; none_mask may be NULL.
 */
int magot_orf6_sizes(const uint64_t* seq_off, uint64_t n, uint64_t* stream_off,
                     uint64_t* stream_len, uint8_t* none_mask);
/* magot_orf6_batch: stream_off must be exactly magot_orf6_sizes' table for
 * seq_off (the kernel places every stream from its record's block start and
 * length); any other table is refused with MAGOT_ERR_ARG before a launch. */
int magot_orf6_batch(magot_ctx* ctx, const uint8_t* seqs, const uint64_t* seq_off, uint64_t n,
                     const uint8_t* lut64, const uint64_t* stream_off, uint8_t* out);
/* Debug: magot_orf6_batch with its device output filled with the byte
 * `poison` (0..255) before the launch, so that a chunk no lane wrote shows in
 * out; poison < 0 fills nothing (magot_orf6_batch itself). */
int magot_debug_orf6_batch(magot_ctx* ctx, const uint8_t* seqs, const uint64_t* seq_off, uint64_t n,
                           const uint8_t* lut64, const uint64_t* stream_off, uint8_t* out,
                           int32_t poison);
/* The same over an extraction plan's records, in HBM (BASELINE configs[4],
 * C5): one kernel gathers each record from the packed genome through the
 * plan's intervals and writes its six translations (the plan's nucleotide
 * output is not needed).  The kernel walks the records in genome order and
 * lays their six-stream blocks out in that order (its stores then stream
 * through the output): stream j is at the stream_off[j] magot_orf6_fetch
 * returns (16-byte aligned, stream_len[j] residues, zero padding), a record's
 * six streams form one contiguous block in the same strand-major order as
 * magot_orf6_sizes, and stream_off[6n] is the total.  MAGOT_ORF6_ORDER=record
 * keeps record order (then stream_off equals magot_orf6_sizes'). */
typedef struct magot_orf6 magot_orf6;
int magot_plan_orf6(magot_ctx* ctx, magot_plan* p, const uint8_t* lut64, magot_orf6** out,
                    uint64_t* total_res);
int magot_orf6_execute(magot_ctx* ctx, magot_orf6* o);
/* Debug: fill the plan's output (total_res bytes) with `byte` on the context
 * stream.  magot_orf6_execute does not clear its output, so without this a
 * chunk that no lane wrote keeps what an earlier execute left there. */
int magot_orf6_poison(magot_ctx* ctx, magot_orf6* o, uint8_t byte);
int magot_orf6_fetch(magot_ctx* ctx, magot_orf6* o, uint8_t* out, uint64_t* stream_off,
                     uint64_t* stream_len);
/* D2D copy of the padded residue bytes (total_res) into caller device memory
 * (e.g. the buffer an output gather sends). */
int magot_orf6_copy_outputs(magot_ctx* ctx, magot_orf6* o, void* dst_dev);
int magot_orf6_time(magot_ctx* ctx, magot_orf6* o, int iters, double* avg_ms);
int magot_orf6_time_b2b(magot_ctx* ctx, magot_orf6* o, int iters, double* avg_ms);
void magot_orf6_destroy(magot_orf6* o);

/*
 * ORF calling over the streams of an executed magot_orf6, where they lie in
 * HBM: dna2orfs (genome_tools.py:145-180) once its contigs are Sequences.
 * A record's streams are visited in the reference's loop order j = 2*frame +
 * (strand == '+') (genome_tools.py:155-156), a frame-0 stream without one
 * leading 'X' (genome.py:819-821); a stream of n residues with s stops gives
 * s + 1 ORFs, empty ones included (split('*'), genome_tools.py:157).  ORF
 * number i of a stream starts at residue k, one past the stop before it (0
 * for the first); its position is (frame on '+', record length - frame on
 * '-') + 3 * k (genome_tools.py:158-164).  The output string is the ORF, or
 * with MAGOT_ORF_FROM_ATG 'M' + what follows its first 'M' with every further
 * 'M' removed, 'M' alone when it has none (genome_tools.py:165-169).  A stream
 * whose translate() is None (record length <= 2 + frame) has no ORFs and
 * flags its record (MAGOT_ORF_REC_NONE: the reference raises AttributeError
 * there).  With MAGOT_ORF_LONGEST each record keeps the first ORF in loop
 * order whose output string is longest (genome_tools.py:172-175); a record
 * all of whose strings are empty has no candidate and is flagged
 * (MAGOT_ORF_REC_NO_LONGEST: the reference's IndexError, genome_tools.py:179),
 * and there is one row per unflagged record.
 *   magot_orfcall_create  runs the passes (o must have been executed, else
 *       MAGOT_ERR_STATE; o must outlive the handle) and reports the table's
 *       rows and the payload's bytes.
 *   magot_orfcall_fetch   the rows, in the plan's record order and loop order
 *       inside a record whatever order the six-frame kernel laid the streams
 *       out in: record, stream j, start residue k, output length, offset in
 *       the concatenated payload; the payload; one flag byte per record.  Any
 *       pointer may be NULL.
 *   magot_orfcall_text    the tool's FASTA text in one device buffer: per row
 *       '>' name '-pos:' position '\n' string '\n' (genome_tools.py:177), or
 *       with MAGOT_ORF_LONGEST '>' name '_longestORF\n' string '\n'
 *       (genome_tools.py:174).  Record r's name is names[name_off[r],
 *       name_off[r+1]) (any bytes).  *out_len receives the size;
 *       magot_orfcall_text_fetch copies the text down (one D2H).
 *   magot_orfcall_time    mean device time of the calling passes (text == 0)
 *       or of the text passes of the last magot_orfcall_text (text != 0),
 *       an event pair around each of `iters` runs.
 * magot_orfcall_tile: residues per tile of the calling passes (an ORF may
 * span any number of tiles).
 */
#define MAGOT_ORF_FROM_ATG 1u
#define MAGOT_ORF_LONGEST 2u
#define MAGOT_ORF_REC_NONE 1u
#define MAGOT_ORF_REC_NO_LONGEST 2u
typedef struct magot_orfcall magot_orfcall;
uint32_t magot_orfcall_tile(void);
int magot_orfcall_create(magot_ctx* ctx, magot_orf6* o, uint32_t flags, magot_orfcall** out,
                         uint64_t* n_orfs, uint64_t* payload_bytes);
int magot_orfcall_fetch(magot_ctx* ctx, magot_orfcall* c, uint32_t* record, uint8_t* stream,
                        uint32_t* start, uint32_t* length, uint64_t* payload_off,
                        uint8_t* payload, uint8_t* record_flags);
int magot_orfcall_text(magot_ctx* ctx, magot_orfcall* c, const uint64_t* name_off,
                       const uint8_t* names, uint64_t* out_len);
int magot_orfcall_text_fetch(magot_ctx* ctx, magot_orfcall* c, uint8_t* out, uint64_t cap);
int magot_orfcall_time(magot_ctx* ctx, magot_orfcall* c, int text, int iters, double* avg_ms);
void magot_orfcall_destroy(magot_orfcall* c);

/*
 * The longest ORF of every record of an executed extraction plan, fused:
 * Sequence.get_orfs(longest=True) (genome.py:824-851) over the plan's
 * nucleotide output where it lies in HBM, as get_CDS_peptides asks it of every
 * CDS (genome_tools.py:283-321).  A record's bytes are what get_seq() returns.
 * Stream j = 2*frame + (strand == '+') of a record of L bases holds the real
 * codons only, (L - 2*frame) / 3 of them when L >= 2*frame + 3 (the definition
 * above magot_orf6_sizes); a residue is lut64[codon] (NULL: the standard
 * code), 'X' when a base is not one of ACGTacgt; a frame-0 stream loses one
 * leading 'X' and its residue indices count from the trimmed start.  A None
 * or empty stream is passed over, as get_orfs passes it over (no
 * MAGOT_ORF_REC_NONE here).  The winner of a record is the first maximal run
 * of residues other than '*', in order of j and then of its start, whose
 * length is the greatest; a record without a non-empty run has none and is
 * flagged MAGOT_ORF_REC_NO_LONGEST (the reference's IndexError,
 * genome.py:849).  No stream, ORF table or losing ORF is written to memory.
 *   magot_longorf_create   p must have MAGOT_OUT_NUC (else MAGOT_ERR_ARG) and
 *       have been executed (else MAGOT_ERR_STATE), in either layout, and must
 *       outlive the handle; a record of 2^32 bases or more: MAGOT_ERR_RANGE.
 *   magot_longorf_execute  the calling pass, a scan of the winners' lengths
 *       and the pass that writes them; reports the payload's bytes.
 *   magot_longorf_fetch    one row per record, in record order: stream j,
 *       start residue k, length (0 for a flagged record), offset in the
 *       concatenated payload; the payload; one flag byte per record.  Any
 *       pointer may be NULL.
 *   magot_longorf_text     the tool's text in one device buffer, for records
 *       [0, n_print): '>' name '\n' residues '\n' (genome_tools.py:318).
 *       Record r's name is names[name_off[r], name_off[r+1]) (any bytes).  A
 *       flagged record among them gets an empty residue line.  *out_len
 *       receives the size; magot_longorf_text_fetch copies the text down.
 *   magot_longorf_time     mean device time of the calling passes (text == 0)
 *       or of the text passes of the last magot_longorf_text (text != 0), an
 *       event pair around each of `iters` runs.
 *   magot_longorf_params   the codons per step of the calling pass (a run may
 *       span any number of steps) and the waves the handle launches, each of
 *       which strides over the records; with h NULL the most any handle of
 *       the context launches.
 */
typedef struct magot_longorf magot_longorf;
int magot_longorf_create(magot_ctx* ctx, magot_plan* p, const uint8_t* lut64, magot_longorf** out);
int magot_longorf_execute(magot_ctx* ctx, magot_longorf* h, uint64_t* payload_bytes);
int magot_longorf_fetch(magot_ctx* ctx, magot_longorf* h, uint8_t* stream, uint32_t* start,
                        uint32_t* length, uint64_t* payload_off, uint8_t* payload,
                        uint8_t* record_flags);
int magot_longorf_text(magot_ctx* ctx, magot_longorf* h, const uint64_t* name_off,
                       const uint8_t* names, uint64_t n_print, uint64_t* out_len);
int magot_longorf_text_fetch(magot_ctx* ctx, magot_longorf* h, uint8_t* out, uint64_t cap);
int magot_longorf_time(magot_ctx* ctx, magot_longorf* h, int text, int iters, double* avg_ms);
int magot_longorf_params(magot_ctx* ctx, const magot_longorf* h, uint32_t* step, uint64_t* waves);
void magot_longorf_destroy(magot_longorf* h);

/*
 * Native batch planner for gff2fasta (genome_tools.py:324-330).
 * Parses GFF3/GTF text with read_gff's rules and default arguments
 * (genome.py:242-415: '#'/8-tab acceptance, version sniffing, ID synthesis
 * and de-duplication, v2 parent hierarchy, Base/Parent typing), keeps the
 * AnnotationSet model (global ID lookup: last matching type in sorted order,
 * genome.py:536-544) and lowers AnnotationSet.get_fasta(feature)
 * (genome.py:578-582, 677-731) to interval and record tables for
 * magot_plan_create plus a FASTA text skeleton.
 * seqids / contig_lens: the GenomeSequence (genome.py:854-877) in the order
 * its contigs were given to magot_genome_load.  flags: MAGOT_GFF_PROTEIN for
 * seq_type="protein", MAGOT_GFF_ORDER_PY2 for CPython 2.7 dict order,
 * MAGOT_GFF_GENOMIC for genomic=True (genome.py:680-682: one '+' interval per
 * feature over its get_coords() span, never translated, so the plan is a
 * nucleotide plan whatever MAGOT_GFF_PROTEIN says), MAGOT_GFF_LONGEST for
 * longest=True (genome.py:720-724: the child record with the longest
 * sequence, the later one on a tie).  For protein the lengths depend on the
 * leading-'X' trim, i.e. on the genome: every candidate is planned and
 * magot_gffplan_render picks (magot_gffplan_selections > 0; such a plan has
 * no device text assembly).  MAGOT_GFF_FROM_EXONS: gff2fasta's
 * from_exons="True" reading (genome_tools.py:326-327: "\texon\t" replaced by
 * "\tCDS\t" in each line, then every type that is a substring of "CDS"
 * ignored).
 * Returns MAGOT_ERR_UNSUPPORTED when the input would take one of the
 * reference's diagnostic paths (prints, None, exceptions): the caller then
 * uses the object path, which reproduces them.
 */
#define MAGOT_GFF_PROTEIN 1u
#define MAGOT_GFF_ORDER_PY2 2u
#define MAGOT_GFF_LONGEST 4u
#define MAGOT_GFF_GENOMIC 8u
#define MAGOT_GFF_FROM_EXONS 16u
#define MAGOT_GFF_FOR_WRITE 32u
typedef struct magot_gffplan magot_gffplan;
int magot_gff_plan(const char* gff, uint64_t gff_len, const char* const* seqids,
                   const uint64_t* contig_lens, uint32_t n_contigs, const char* feature,
                   uint32_t flags, magot_gffplan** out, uint64_t* n_exons, uint64_t* n_tx);
/*
 * magot_gff_plan in two steps, so the GFF can be read before the genome's
 * contig names are known (gff2fasta reads the GFF while another thread
 * loads the FASTA): magot_gff_read is read_gff (genome.py:242-415; flags:
 * MAGOT_GFF_FROM_EXONS is the only one it looks at), magot_gff_lower the
 * get_fasta lowering against the contigs (the other flags, as above; once
 * per plan, else MAGOT_ERR_STATE).  `gff` must stay valid until
 * magot_gff_lower returns.  Either returns MAGOT_ERR_UNSUPPORTED for a
 * diagnostic path; the plan handle from magot_gff_read is then still the
 * caller's to destroy.  MAGOT_GFF_FOR_WRITE (not with MAGOT_GFF_FROM_EXONS:
 * MAGOT_ERR_ARG) makes magot_gff_read keep, per feature, what
 * magot_gff_lower_write needs; without it the model is what it always was.
 */
int magot_gff_read(const char* gff, uint64_t gff_len, uint32_t flags, magot_gffplan** out);
int magot_gff_lower(magot_gffplan* p, const char* const* seqids, const uint64_t* contig_lens,
                    uint32_t n_contigs, const char* feature, uint32_t flags, uint64_t* n_exons,
                    uint64_t* n_tx);
/*
 * get_CDS_peptides (genome_tools.py:283-321, its read_gff3 read as read_gff)
 * lowered from a plan magot_gff_read made (once per plan, else
 * MAGOT_ERR_STATE): one single-interval record per printed CDS in output
 * order (magot_gffplan_tables; start_rc clamped as the Python slice clamps,
 * bit 63 from the CDS's own strand, '.' counting as '+'), and the records'
 * names.  Genes come in the order of annotations.gene (flags:
 * MAGOT_GFF_ORDER_PY2, as magot_gff_lower).  A gene is dropped when one of the
 * n_filters strings is a substring of its ID, or when length_filter is not
 * NULL and the first record of its get_fasta() has fewer bases.  Per
 * transcript of a kept gene the CDS children are keyed by coords (a later one
 * replaces an earlier one), sorted, and reversed when the transcript's strand
 * is '-'.  names_from: the CDS's ID, or the transcript's or the gene's ID +
 * "-CDS" + n, n counted from 1 per transcript.  The records of one transcript
 * form a group: the reference computes every ORF of a transcript before it
 * writes the first, so an IndexError (MAGOT_ORF_REC_NO_LONGEST from
 * magot_longorf) cuts the output at the start of its record's group.
 * MAGOT_ERR_UNSUPPORTED whenever anything in the annotation, dropped genes
 * included, would take the reference off its straight path (a gene child that
 * is no transcript, a transcript child that is no CDS, a seqid the genome does
 * not have, a strand outside + - ., a gene whose get_fasta() has no second
 * line, a replaced CDS on another seqid than the one that replaces it): the
 * object path reproduces those.  The gene, transcript and CDS dicts themselves
 * are missing only where read_gff returns None and leaves no annotations at
 * all (AttributeError in the reference): magot_gff_read declines such a text,
 * so it never reaches this call; a model that was read always has the three.
 *   magot_gffplan_cds_views  name_off (n_rec + 1) into names, and group_off
 *       (n_groups + 1) into the records; valid while the plan lives.
 */
#define MAGOT_CDS_NAMES_CDS 0u
#define MAGOT_CDS_NAMES_TRANSCRIPT 1u
#define MAGOT_CDS_NAMES_GENE 2u
int magot_gff_lower_cds(magot_gffplan* p, const char* const* seqids, const uint64_t* contig_lens,
                        uint32_t n_contigs, const char* const* filters, uint32_t n_filters,
                        const int64_t* length_filter, uint32_t names_from, uint32_t flags,
                        uint64_t* n_rec, uint64_t* n_groups);
int magot_gffplan_cds_views(const magot_gffplan* p, const uint64_t** name_off,
                            const uint8_t** names, const uint64_t** group_off);
/*
 * extract_upstream_downstream (genome_tools.py:457-480) as a plan of the same
 * shape: one single-interval record per printed window (the `sequence_length`
 * bases before a '+' feature for stream "up", after it reverse-complemented
 * for "down"; mirrored on '-'), names from the last `namefrom=` attribute or
 * "seq<k>", a matching line whose strand is neither '+' nor '-' repeating the
 * previous window, windows shorter than sequence_length dropped, records
 * joined by "\n".  Render it with magot_gffplan_render or magot_fasta_text_*
 * like a gff2fasta plan (nucleotide).  sequence_length is the reference's
 * string argument.  MAGOT_ERR_UNSUPPORTED when the reference would raise
 * (unknown seqid, a bad integer, `namefrom` without '=', no window yet).
 */
int magot_flank_plan(const char* gff, uint64_t gff_len, const char* const* seqids,
                     const uint64_t* contig_lens, uint32_t n_contigs, const char* feature_type,
                     const char* namefrom, const char* sequence_length, const char* stream,
                     magot_gffplan** out, uint64_t* n_exons, uint64_t* n_tx);
/* Copy the planned tables (n_exons / n_tx entries from magot_gff_plan). */
int magot_gffplan_tables(const magot_gffplan* p, magot_exon* exons, magot_tx* txs);
/* The planned tables in place (n_exons / n_tx rows, valid until the plan is
 * destroyed; NULL when empty): magot_plan_create reads them without a copy. */
int magot_gffplan_table_views(const magot_gffplan* p, const magot_exon** exons,
                              const magot_tx** txs);
/* The FASTA text: skeleton + record payloads from magot_plan_fetch (nuc for
 * nucleotide plans, untrimmed pep for protein; the leading-'X' trim of
 * genome.py:819-821 is applied here).  out == NULL: *out_len = size only. */
int magot_gffplan_render(const magot_gffplan* p, const uint8_t* nuc, const uint64_t* noff,
                         const uint8_t* pep, const uint64_t* poff, uint8_t* out, uint64_t cap,
                         uint64_t* out_len);
/* Number of longest=True protein choices the render makes (0: none). */
int magot_gffplan_selections(const magot_gffplan* p, uint64_t* n_groups);
void magot_gffplan_destroy(magot_gffplan* p);

/*
 * The same FASTA text assembled on device: the skeleton of
 * `gp` is uploaded once, and each execute fills it with the payloads of
 * extraction plan `p` (built from gp's tables, with MAGOT_OUT_PEP for a
 * protein skeleton, MAGOT_OUT_NUC otherwise) in one device buffer: per-unit
 * lengths (trimX applied), a scan, and a copy kernel.  fetch synchronises and
 * copies the *out_len bytes (out == NULL: length only).  max_bytes bounds
 * *out_len.  p must outlive the handle.  Replaces the text building of
 * AnnotationSet.get_fasta / ParentAnnotation.get_fasta
 * (genome.py:578-582, 677-731) for the gff2fasta CLI (genome_tools.py:330).
 */
typedef struct magot_fasta_text magot_fasta_text;
int magot_fasta_text_create(magot_ctx* ctx, const magot_gffplan* gp, const magot_plan* p,
                            magot_fasta_text** out, uint64_t* max_bytes);
int magot_fasta_text_execute(magot_ctx* ctx, magot_fasta_text* t);
int magot_fasta_text_fetch(magot_ctx* ctx, magot_fasta_text* t, uint8_t* out, uint64_t cap,
                           uint64_t* out_len);
int magot_fasta_text_time(magot_ctx* ctx, magot_fasta_text* t, int iters, double* avg_ms);
void magot_fasta_text_destroy(magot_fasta_text* t);

/*
 * mask_from_gff (genome_tools.py:394-428): every base under a GFF feature of
 * one type lower-cased (soft) or replaced by 'N' (MAGOT_MASK_HARD), after the
 * whole genome was upper-cased unless MAGOT_MASK_KEEP_CASE (the reference's
 * overwrite_softmask "False"); both case changes are ASCII-only.
 *
 * Host planner (genome_tools.py:410-426).  magot_mask_plan scans the GFF text:
 * every line with more than five tabs counts, '#' lines included
 * (genome_tools.py:412); a line is used when fields[2] == feature_type
 * (:414); int(fields[3]) and int(fields[4]) are read as magot_flank_plan reads
 * them (:415-416).  The table holds {contig, 0-based start, length} pieces of
 * the slices lst[start - 1:stop] (:418, :423), clipped to the contig, lines
 * that change nothing dropped, in GFF order, unsorted and unmerged; a slice
 * longer than magot_mask_piece() bases is cut into pieces of at most that
 * many, so no device lane owns more.  In-range features are idempotent and
 * commute, so the table is exact however they overlap.  MAGOT_ERR_UNSUPPORTED
 * where the reference's sequential replay matters: a bad integer
 * (ValueError), an unknown fields[0] (KeyError), a negative slice index
 * (start < 1 or stop < 0) on a line that changes anything, a hard mask that
 * changes the list's length (stop > len with start <= stop, :420-423).  The
 * caller's line loop reproduces those.  seqids / contig_lens as for
 * magot_gff_plan; contigs of 4 Gbases or more are refused (MAGOT_ERR_ARG).
 *   magot_maskplan_table   the rows in place (valid until destroy; NULL when
 *       empty), their count and the plan's flags; any pointer may be NULL.
 *   magot_mask_fasta_check MAGOT_OK when the n_contigs contigs the native
 *       reader (magot_genome_load_fasta / magot_fasta_read, truncate_names)
 *       found in `text` are the entries the reference's own read loop builds
 *       (genome_tools.py:398-409); MAGOT_ERR_UNSUPPORTED for sequence before
 *       the first header (KeyError, :404), whitespace directly after '>' (the
 *       name is line.split()[0][1:], :400), an empty contig (kept and
 *       printed, :401) or a repeated name (reset, :401).
 *
 * Device object (genome_tools.py:427-428: '>' name '\n' sequence '\n' per
 * contig, the sequence on one line).  `p` is a nucleotide extraction plan
 * with one record per contig of the output, in output order, each gathering
 * its contig whole on '+' (record r is contig rec_contig[r]; every contig of
 * the mask plan in exactly one record, lengths checked); it reproduces every
 * input byte.  Record r's name is names[name_off[r], name_off[r+1]).
 *   magot_mask_create   uploads the pieces and headers and sizes the buffers;
 *       *text_bytes is the size of the final text.  p must outlive the
 *       handle; mp may be destroyed on return.
 *   magot_mask_execute  enqueues, on the context stream, the zeroing of the
 *       coverage plane (one bit per byte of p's nucleotide output),
 *       mask_paint_kernel and mask_text_kernel (p must have been executed,
 *       else MAGOT_ERR_STATE).
 *   magot_mask_fetch    synchronises and copies the text down (one D2H).
 *   magot_mask_coverage_fetch  the plane's words (bit i of word w = byte
 *       32 * w + i of p's output, which holds record r at magot_plan_layout's
 *       nuc_start[r]); *n_words alone when words == NULL.  For tests.
 *   magot_mask_time     mean device time over `iters` runs of the zeroing +
 *       paint (paint_ms) and of the text kernel (text_ms), an event pair
 *       around each.
 */
#define MAGOT_MASK_HARD 1u
#define MAGOT_MASK_KEEP_CASE 2u
typedef struct magot_mask_interval {
  uint32_t contig;
  uint32_t start;
  uint32_t len;
} magot_mask_interval;
typedef struct magot_maskplan magot_maskplan;
typedef struct magot_mask magot_mask;
uint32_t magot_mask_piece(void);
int magot_mask_plan(const char* gff, uint64_t gff_len, const char* const* seqids,
                    const uint64_t* contig_lens, uint32_t n_contigs, const char* feature_type,
                    uint32_t flags, magot_maskplan** out, uint64_t* n_intervals);
int magot_maskplan_table(const magot_maskplan* p, const magot_mask_interval** rows,
                         uint64_t* n_intervals, uint32_t* flags);
void magot_maskplan_destroy(magot_maskplan* p);
int magot_mask_fasta_check(const char* text, uint64_t len, uint32_t n_contigs);
int magot_mask_create(magot_ctx* ctx, const magot_plan* p, const magot_maskplan* mp,
                      const uint32_t* rec_contig, const uint64_t* name_off, const uint8_t* names,
                      magot_mask** out, uint64_t* text_bytes);
int magot_mask_execute(magot_ctx* ctx, magot_mask* m);
int magot_mask_fetch(magot_ctx* ctx, magot_mask* m, uint8_t* out, uint64_t cap);
int magot_mask_coverage_fetch(magot_ctx* ctx, magot_mask* m, uint32_t* words, uint64_t cap_words,
                              uint64_t* n_words);
int magot_mask_time(magot_ctx* ctx, magot_mask* m, int iters, double* paint_ms, double* text_ms);
void magot_mask_destroy(magot_mask* m);

/*
 * position_dic (genome.py:981-1100) on the device: a bit track over a packed
 * genome, one bit per base in the genome's forward coordinates (bit g & 31 of
 * word g >> 5; contig c's base i is coordinate 64 + the lengths of the contigs
 * before c + i); every bit outside the contigs is 0.  All passes run on the
 * context stream.  The genome must outlive the track, the track its windows.
 *   magot_track_create      a zeroed track over g; *n_words = its words.
 *   magot_track_base_class  the A/T class (genome.py:1029: byte in "ATat") or,
 *       with MAGOT_TRACK_GC, the C/G class of g's bases, OR-ed into the track
 *       or, with MAGOT_TRACK_REPLACE, replacing it.  g must be the genome the
 *       track was created over (MAGOT_ERR_ARG).
 *   magot_track_paint       sets (value 1) or clears (value 0) the bases under
 *       interval pieces {contig, 0-based start, len <= the mask piece}; rows
 *       may overlap, nest and repeat.  A row outside its contig is
 *       MAGOT_ERR_RANGE, a longer one MAGOT_ERR_ARG, before any launch.
 *   magot_track_set_bytes / _get_bytes   one contig's bits from / to one byte
 *       per base (any non-zero byte sets the bit; 0 / 1 come back): a numpy
 *       bool array.  len must be the contig's length.
 *   magot_track_fetch       the words; *n_words alone when words == NULL.
 *   magot_track_windows_create   sliding windows (genome.py:1043-1053): contig
 *       c has (len - window) / jump windows when len > window and skip[c] is 0
 *       (skip may be NULL), else none; window i covers bases [i * jump,
 *       i * jump + window).  Enqueues the sums (one rank difference per
 *       window; the rank directory is rebuilt first when a producer ran since).
 *       *n_windows = their total, first[c] (n_contigs + 1 entries) contig c's
 *       first window.  window and jump must be >= 1 (MAGOT_ERR_ARG).
 *   magot_track_windows_fetch    the sums, in window order.
 *   magot_track_transitions      the windows whose test sum >= s_min differs
 *       from the previous window's of the same contig (false before a contig's
 *       first window), counted and written on the device; *n = how many.
 *   magot_track_transitions_fetch   their window indices, ascending
 *       (MAGOT_ERR_STATE before magot_track_transitions).
 *   magot_track_count       ones[i] = set bits under row i (any length).
 *   magot_track_time        mean device ms over `iters` runs of: the A/T class
 *       pass (into a scratch plane), the rank directory, the window sums, the
 *       transitions (count, scan, write) and one whole-contig count per
 *       contig, in ms5[0..4]; w may be NULL (entries 2 and 3 are then 0).
 *   magot_track_rank_block  bases per rank directory block.
 */
#define MAGOT_TRACK_GC 1u
#define MAGOT_TRACK_REPLACE 2u
typedef struct magot_track magot_track;
typedef struct magot_track_windows magot_track_windows;
uint32_t magot_track_rank_block(void);
int magot_track_create(magot_ctx* ctx, const magot_genome* g, magot_track** out,
                       uint64_t* n_words);
int magot_track_base_class(magot_ctx* ctx, magot_track* t, const magot_genome* g, uint32_t flags);
int magot_track_paint(magot_ctx* ctx, magot_track* t, const magot_mask_interval* rows,
                      uint64_t n_rows, int value);
int magot_track_set_bytes(magot_ctx* ctx, magot_track* t, uint32_t contig, const uint8_t* bytes,
                          uint64_t len);
int magot_track_get_bytes(magot_ctx* ctx, magot_track* t, uint32_t contig, uint8_t* bytes,
                          uint64_t len);
int magot_track_fetch(magot_ctx* ctx, magot_track* t, uint32_t* words, uint64_t cap_words,
                      uint64_t* n_words);
int magot_track_windows_create(magot_ctx* ctx, magot_track* t, uint64_t window, uint64_t jump,
                               const uint8_t* skip, magot_track_windows** out,
                               uint64_t* n_windows, uint64_t* first);
int magot_track_windows_fetch(magot_ctx* ctx, magot_track_windows* w, uint32_t* sums,
                              uint64_t cap);
int magot_track_transitions(magot_ctx* ctx, magot_track_windows* w, uint32_t s_min, uint64_t* n);
int magot_track_transitions_fetch(magot_ctx* ctx, magot_track_windows* w, uint64_t* index,
                                  uint64_t cap);
int magot_track_count(magot_ctx* ctx, magot_track* t, const magot_mask_interval* rows,
                      uint64_t n_rows, uint32_t* ones);
int magot_track_time(magot_ctx* ctx, magot_track* t, magot_track_windows* w, uint32_t s_min,
                     int iters, double* ms5);
void magot_track_windows_destroy(magot_track_windows* w);
void magot_track_destroy(magot_track* t);

/*
 * depth_from_gff (genome_tools.py:598-652) on the device: the depth column of
 * a `samtools depth` table as one int32 per line, and interval sums over it.
 *
 * Grammar of a line: name SEP pos SEP depth (SEP token)* [SEP] [CR] LF; SEP
 * one or more of space and tab; name 1..255 bytes of 0x21..0x7E; pos and depth
 * 1..10 digits, value <= 2^31 - 1; the last line may lack its LF.  A line
 * whose name differs from the line before starts a run; line k (from 0) of a
 * run must have pos k + 1; no two runs carry one name.  For such a table the
 * reference's array of a contig is the depth column of its run.
 *   magot_depth_parse   streams the text in chunks of about chunk_bytes (0: a
 *       default sized for transfer; cut after an LF) through pinned staging,
 *       each upload overlapped with the parse of the chunk before, and builds
 *       the sum directory.  A table outside the grammar is declined: *out =
 *       NULL, *reason a MAGOT_DEPTH_* code and *line the first offending line
 *       (1-based; 0 for the two whole-table limits).  Otherwise *reason = 0,
 *       *n_lines and *n_runs describe the track.  max_runs 0: 2^20.
 *   magot_depth_runs    the runs in file order: first line (0-based), offset
 *       of the name in the text, name length.
 *   magot_depth_values  lines [start, start + n) of the depth column.
 *   magot_depth_sums    sums[i] = the sum of lines [start[i], start[i] +
 *       length[i]) (0 when length[i] <= 0; otherwise a row outside the table
 *       is MAGOT_ERR_RANGE, before any launch); with group_offsets (n_groups +
 *       1 ascending entries, a CSR over the rows) also group_sums[g] = the sum
 *       of its rows' sums.  group_offsets and group_sums may be NULL.
 *   magot_depth_time    mean device ms over `iters` runs of: the line index
 *       and the parse of the last chunk (still on the device; *chunk_len its
 *       bytes), the directory, and one whole-run sum per run, in ms4[0..3].
 *   magot_depth_block   depths per directory block.
 */
#define MAGOT_DEPTH_EMPTY_LINE 1u
#define MAGOT_DEPTH_LEADING_BLANK 2u
#define MAGOT_DEPTH_BAD_BYTE 3u
#define MAGOT_DEPTH_NAME_LONG 4u
#define MAGOT_DEPTH_FEW_FIELDS 5u
#define MAGOT_DEPTH_SIGN 6u
#define MAGOT_DEPTH_NOT_NUMBER 7u
#define MAGOT_DEPTH_NUMBER_RANGE 8u
#define MAGOT_DEPTH_POS_SEQUENCE 9u
#define MAGOT_DEPTH_REPEATED_CONTIG 10u
#define MAGOT_DEPTH_LINE_LONG 11u /* a line longer than a chunk */
#define MAGOT_DEPTH_TOO_MANY_LINES 12u
#define MAGOT_DEPTH_TOO_MANY_RUNS 13u
typedef struct magot_depth magot_depth;
uint32_t magot_depth_block(void);
int magot_depth_parse(magot_ctx* ctx, const char* text, uint64_t len, uint64_t chunk_bytes,
                      uint32_t max_runs, magot_depth** out, uint64_t* n_lines, uint64_t* n_runs,
                      uint32_t* reason, uint64_t* line);
int magot_depth_runs(const magot_depth* t, uint64_t* first, uint64_t* offset, uint32_t* name_len,
                     uint64_t cap);
int magot_depth_values(magot_ctx* ctx, magot_depth* t, uint64_t start, uint64_t n, int32_t* out);
int magot_depth_sums(magot_ctx* ctx, magot_depth* t, const int64_t* start, const int64_t* length,
                     uint64_t n_rows, const uint64_t* group_offsets, uint64_t n_groups,
                     int64_t* sums, int64_t* group_sums);
int magot_depth_time(magot_ctx* ctx, magot_depth* t, int iters, double* ms4,
                     uint64_t* chunk_len);
void magot_depth_destroy(magot_depth* t);

/*
 * fqstats (genome_tools.py:85-124) on the device: the lengths of a FASTQ's
 * sequence lines as a histogram, and the tool's figures from it.
 *
 * A line ends at LF only; line k (from 0) is a sequence line when k % 4 == 1,
 * whatever it holds; its length is its bytes without the LF (a CR counts), and
 * one less than its bytes for a last line without LF.  Lines may be of any
 * length; no text is declined.
 *   magot_fq_dense      lengths below it are counted in one uint64 bin each,
 *       longer ones kept in a list.
 *   magot_fq_parse      streams the text in chunks of chunk_bytes (0: a default
 *       sized for transfer; 1 KB at the least, 1 GB at the most; cut anywhere,
 *       in a line or between a CR and its LF) through pinned staging, each upload
 *       overlapped with the passes over the chunk before, and reduces the
 *       histogram to the figures on the device.
 *   magot_fq_stats      out8: reads, bases, desc[reads / 2], desc[reads / 4],
 *       desc[reads * 3 / 4] (desc: the lengths in descending order), and n25,
 *       n50, n75: the first length of desc at which the running sum is above
 *       bases / 4, bases / 2, bases * 3 / 4.  Bit k of *flags: n25 / n50 / n75
 *       (k = 0, 1, 2) was set (never when bases is 0).  With no reads
 *       everything but out8[0] is 0.
 *   magot_fq_histogram  the lengths that occur, ascending, and how often:
 *       *n entries; with lengths and counts NULL only *n is set, otherwise
 *       cap must be at least *n.
 *   magot_fq_time       mean device ms over `iters` runs of: the line index and
 *       the length pass of the last chunk (still on the device; *chunk_len its
 *       bytes; into a histogram of their own), the reduction, and a device
 *       copy of chunk_len bytes, in ms4[0..3].
 */
typedef struct magot_fq magot_fq;
uint64_t magot_fq_dense(void);
int magot_fq_parse(magot_ctx* ctx, const char* text, uint64_t len, uint64_t chunk_bytes,
                   magot_fq** out);
int magot_fq_stats(const magot_fq* t, uint64_t* out8, uint32_t* flags);
int magot_fq_histogram(magot_ctx* ctx, magot_fq* t, int64_t* lengths, uint64_t* counts,
                       uint64_t cap, uint64_t* n);
int magot_fq_time(magot_ctx* ctx, magot_fq* t, int iters, double* ms4, uint64_t* chunk_len);
void magot_fq_destroy(magot_fq* t);

/* ---- interval joins: purge_overlaps, annotation_overlap ----
 * (genome_tools.py:548-568, annotation_funcs.py:13-30).  An index over a set
 * of intervals (dense seqid, p0, p1), the integers as parsed: nothing is
 * sorted by the caller, ordered or clipped; reversed and negative coordinates
 * are legal.  Each query (seqid, c0, c1) is answered from sorted tables by
 * binary search; a seqid not below n_seq (MAGOT_OVERLAP_NO_SEQ) has no
 * partner.
 *   magot_overlap_coord_range  the coordinates an index holds, [-2^39, 2^39);
 *       one outside is MAGOT_ERR_RANGE before any launch.
 *   magot_overlap_lane_scan    overlap's range scan: a query with more
 *       intervals starting inside it is scanned by a whole wave.
 *   magot_overlap_create   uploads the intervals and builds the tables on the
 *       context stream (n_seq below 2^24).
 *   magot_overlap_purge    drop[i] = 1 when any interval p of query i's seqid
 *       has p0 < c0 < p1, p0 < c1 < p1 or c0 < p0 < c1 (all strict).
 *   magot_overlap_counts   counts[i] = the intervals p of query i's seqid with
 *       p0 <= q0 <= p1 or p0 <= q1 <= p1 (closed).
 *   magot_overlap_time     mean device ms over `iters` runs of: the key pass,
 *       the five sorts, the segment bounds, the purge pass and the overlap
 *       passes over the last query set given (0 when none was), and a device
 *       copy of the sorted tables (*copy_bytes), in ms6[0..5].
 * Host planner of purge_overlaps.  magot_overlap_plan scans both GFF texts
 * (lines end after '\n' only) into one row per line: whether it has more than
 * 6 tabs, and then the dense seqid of its first column in the first file's
 * dictionary (MAGOT_OVERLAP_NO_SEQ: second file only, not there; its integers
 * are then not read), int(x[3]), int(x[4]) as Python 2 reads them, the line's
 * offset and its length with the LF.  MAGOT_ERR_UNSUPPORTED with *reason set
 * where only the reference's sequential run is exact.
 *   magot_ovplan_table     file `which` (0, 1): the columns in place (valid
 *       until destroy); any pointer may be NULL.
 *   magot_ovplan_render    the second file's lines with drop[line] == 0, each
 *       without its last byte and with '\n' instead, in file order: *bytes
 *       always; the text when out is not NULL (cap >= *bytes).
 */
#define MAGOT_OVERLAP_NO_SEQ 0xffffffffu
enum {
  MAGOT_OVERLAP_BAD_INT_FIRST = 1,  /* ValueError before anything is printed */
  MAGOT_OVERLAP_BAD_INT_SECOND = 2, /* ValueError after part of the output */
  MAGOT_OVERLAP_COORD_RANGE = 3,    /* a coordinate outside magot_overlap_coord_range */
  MAGOT_OVERLAP_SEQIDS = 4          /* 2^24 - 1 seqids or more */
};
typedef struct magot_overlap magot_overlap;
typedef struct magot_ovplan magot_ovplan;
void magot_overlap_coord_range(int64_t* lo, int64_t* hi);
uint32_t magot_overlap_lane_scan(void);
int magot_overlap_create(magot_ctx* ctx, const uint32_t* seq, const int64_t* p0, const int64_t* p1,
                         uint64_t n, uint32_t n_seq, magot_overlap** out);
int magot_overlap_purge(magot_ctx* ctx, magot_overlap* h, const uint32_t* seq, const int64_t* c0,
                        const int64_t* c1, uint64_t n, uint8_t* drop);
int magot_overlap_counts(magot_ctx* ctx, magot_overlap* h, const uint32_t* seq, const int64_t* q0,
                         const int64_t* q1, uint64_t n, int64_t* counts);
int magot_overlap_time(magot_ctx* ctx, magot_overlap* h, int iters, double* ms6,
                       uint64_t* copy_bytes);
void magot_overlap_destroy(magot_overlap* h);
int magot_overlap_plan(const char* gff1, uint64_t len1, const char* gff2, uint64_t len2,
                       magot_ovplan** out, uint32_t* reason);
int magot_ovplan_table(const magot_ovplan* p, int which, uint64_t* n_lines, uint32_t* n_seq,
                       const uint8_t** flag, const uint32_t** seq, const int64_t** c0,
                       const int64_t** c1, const uint64_t** off, const uint64_t** len);
int magot_ovplan_render(const magot_ovplan* p, const char* gff2, uint64_t len2,
                        const uint8_t* drop, uint8_t* out, uint64_t cap, uint64_t* bytes);
void magot_ovplan_destroy(magot_ovplan* p);

/*
 * besthits_from_psl (genome_tools.py:572-592) on the device: per query name of
 * a BLAT PSL the line with the highest matches - misMatches, as a reduction
 * keyed by a string: hash the key, sort, verify the grouping byte for byte,
 * reduce by segment.
 *
 * A line ends at LF only; the last one may lack it.  A line whose first byte is
 * one of 'p', LF, 'm', '-', TAB, space is a pass-through line.  Every other
 * line is a data line: at least 9 tabs; field 0 and field 1 each 1..10 digits,
 * value <= 2^31 - 1, no sign, no blanks; the key is the bytes between the 9th
 * tab and the next tab or the end of the line, the LF (and a CR before it)
 * included when field 9 is the last.  score = field 0 - field 1; of the lines
 * of one key the highest score wins, the earliest line among equals.
 *   magot_psl_parse   uploads the whole text into one device buffer through the
 *       context's pinned ring and runs every pass.  Declined with
 *       MAGOT_ERR_UNSUPPORTED, *out = NULL and *reason a MAGOT_PSL_* code: a
 *       text longer than max_bytes (0: a quarter of the free device memory),
 *       before anything of that size is allocated; more than 2^31 - 1 lines;
 *       a data line outside the grammar (the first such line, 1-based, in
 *       *line; on a line with several faults: few fields, then field 0, then
 *       field 1, form before range); two different keys in one bucket of the
 *       low hash_bits bits (1..64) of CPython 2.7's string hash.  *line is 0
 *       for the whole-text reasons.  A null text with len > 0 and hash_bits
 *       outside 1..64 are MAGOT_ERR_ARG before any launch.
 *   magot_psl_sizes   lines, pass-through lines, data lines, keys.
 *   magot_psl_upload_ms  what the upload took inside magot_psl_parse, in device
 *       ms from its first copy's enqueue to its last byte's arrival: the host's
 *       copies into the pinned ring lie in between.
 *   magot_psl_pass_lines  the pass-through lines in file order: offset in the
 *       text and length, the LF included.
 *   magot_psl_groups  one row per key in first-seen order: the full 64-bit hash
 *       of the key, its first line and its best line (0-based), the best score,
 *       and the best line's offset and length (LF included).  Any pointer may
 *       be NULL.
 *   magot_psl_time    mean device ms over `iters` runs of: the line index, the
 *       parse, the compaction, the sort, the verification, the reduction, the
 *       first-seen order with its gather, and a device copy of the text
 *       (*text_bytes), in ms8[0..7].  The handle's answers stand afterwards.
 * Host side (no device):
 *   magot_psl_order   perm[0..n): the order in which a CPython 2.7 dict iterates
 *       n distinct keys inserted in the order given, from their hashes alone.
 *   magot_psl_render  per row (off, len) of the text the bytes [off, off + len
 *       - 1) and an LF (`print line[:-1]`); with whole != 0 all len bytes and
 *       an LF (`print line`).  *bytes always; the text when out is not NULL
 *       (cap >= *bytes).  A row outside the text, or an empty row without
 *       `whole`, is MAGOT_ERR_RANGE.
 */
enum {
  MAGOT_PSL_FEW_FIELDS = 1,     /* a data line with fewer than 10 fields */
  MAGOT_PSL_INTEGER_FORM = 2,   /* field 0 or 1 is not 1 or more digits alone */
  MAGOT_PSL_NUMBER_RANGE = 3,   /* more than 10 digits, or above 2^31 - 1 */
  MAGOT_PSL_HASH_COLLISION = 4, /* two keys in one bucket of the masked hash */
  MAGOT_PSL_TOO_LARGE = 5,      /* the text is longer than max_bytes */
  MAGOT_PSL_TOO_MANY_LINES = 6  /* more than 2^31 - 1 lines */
};
typedef struct magot_psl magot_psl;
int magot_psl_parse(magot_ctx* ctx, const char* text, uint64_t len, uint32_t hash_bits,
                    uint64_t max_bytes, magot_psl** out, uint32_t* reason, uint64_t* line);
int magot_psl_sizes(const magot_psl* p, uint64_t* n_lines, uint64_t* n_pass, uint64_t* n_data,
                    uint64_t* n_groups);
double magot_psl_upload_ms(const magot_psl* p);
int magot_psl_pass_lines(magot_ctx* ctx, magot_psl* p, uint64_t* off, uint64_t* len);
int magot_psl_groups(magot_ctx* ctx, magot_psl* p, uint64_t* hash, uint32_t* first_line,
                     uint32_t* best_line, int64_t* score, uint64_t* off, uint64_t* len);
int magot_psl_time(magot_ctx* ctx, magot_psl* p, int iters, double* ms8, uint64_t* text_bytes);
void magot_psl_destroy(magot_psl* p);
int magot_psl_order(const uint64_t* hash, uint64_t n, uint64_t* perm);
int magot_psl_render(const char* text, uint64_t len, const uint64_t* off, const uint64_t* row_len,
                     uint64_t n, int whole, uint8_t* out, uint64_t cap, uint64_t* bytes);

/*
 * composition_by_site (genome_tools.py:488-503) on the device: per site of an
 * alignment, how many rows hold a, t, c, g there, either case; every other
 * byte (N, '-', IUPAC, ...) is left out.  The rows are stretches of a resident
 * genome's contigs, so one pass over its forward plane counts them.
 *   magot_site_create  row r is the n_sites bases of contig contig[r] from
 *       offset[r] (0-based); a caller may so count a block of rows or of sites.
 *       n_sites = 0 or n_rows = 0, 2^32 rows or more, and a genome of another
 *       context are MAGOT_ERR_ARG; a row that names no contig or runs past its
 *       contig's end is MAGOT_ERR_RANGE; all before any launch.  The genome
 *       must outlive the handle.
 *   magot_site_execute  the counting pass, on the context stream.
 *   magot_site_counts  n_sites x 4 counts, a, t, c, g per site, to the
 *       caller's buffer (MAGOT_ERR_STATE before magot_site_execute).
 *   magot_site_time    mean device ms over `iters` runs of the pass.
 *   magot_site_params  the pass's shape, for tests that straddle it: sites per
 *       lane and per workgroup tile, rows per strip (above which row strips are
 *       combined with atomics), and the rows after which the 4-bit and the 8-bit
 *       counters are widened.  Any pointer may be NULL.
 * Host side (no device):
 *   magot_site_render  the tool's text from n_sites x 4 counts:
 *       "a\tt\tc\tg\n", then per site the four quotients count / (a + t + c + g)
 *       as Python 2's str(float) prints them ('%.12g'; ".0" appended to a
 *       result without '.' or 'e').  *text is allocated here (n_threads
 *       threads; 0: up to 16) and released with magot_site_text_free.  A site
 *       whose four counts are 0 is MAGOT_ERR_RANGE with the first such site in
 *       *empty_site and no text; otherwise *empty_site = n_sites.
 */
typedef struct magot_site magot_site;
int magot_site_create(magot_ctx* ctx, const magot_genome* g, const uint32_t* contig,
                      const uint64_t* offset, uint64_t n_rows, uint64_t n_sites, magot_site** out);
int magot_site_execute(magot_ctx* ctx, magot_site* p);
int magot_site_counts(magot_ctx* ctx, magot_site* p, uint32_t* counts);
int magot_site_time(magot_ctx* ctx, magot_site* p, int iters, double* ms);
void magot_site_params(uint32_t* sites_per_lane, uint32_t* sites_per_tile, uint32_t* rows_per_strip,
                       uint32_t* widen4_rows, uint32_t* widen8_rows);
void magot_site_destroy(magot_site* p);
int magot_site_render(const uint32_t* counts, uint64_t n_sites, uint32_t n_threads, uint8_t** text,
                      uint64_t* bytes, uint64_t* empty_site);
void magot_site_text_free(uint8_t* text);

/*
 * heterozygosity_from_vcf (magot_variants.py:16-139) on the device: per locus
 * and sample the variants inside whose GT's first and last byte differ.  The
 * text is resident, as a PSL's; spans are (offset, length) into it and leave
 * the line's LF out.
 *   magot_vcf_parse   uploads and indexes the text, places its data lines and
 *       "##" lines, reads S from the '#' line and parses every data line.
 *       Outside the native grammar: MAGOT_ERR_UNSUPPORTED, *out = NULL, *reason
 *       a MAGOT_VCF_* code and *line the 1-based line (0: none).  max_bytes as
 *       magot_psl_parse's; max_samples and max_runs 0 for the limits below, or
 *       less, for tests.
 *   magot_vcf_sizes   lines, data lines, "##" lines, samples, words per bit row,
 *       CHROM runs, and the span of the '#' line.
 *   magot_vcf_header_lines  the spans of the "##" lines in file order.
 *   magot_vcf_runs    the CHROM span of each run's first line: consecutive data
 *       lines with one CHROM are a run.
 *   magot_vcf_resolve contig[r] of each run (the caller's numbering): keys
 *       (contig << 32 | POS), a stable sort, and per data line whether it is the
 *       last (kept) and the first of its key.
 *   magot_vcf_tables  per data line, in file order: its 0-based line, POS, the
 *       CPython 2.7 hash of CHROM<:>POS, kept, first (both after
 *       magot_vcf_resolve, else 0), and the bit rows (data lines x words).
 *       Any pointer may be NULL.
 *   magot_vcf_last_of the 0-based line and span of the kept line whose key is
 *       that of data line d.
 *   magot_vcf_count   per locus (contig, lo, hi: positions lo..hi, none when
 *       lo > hi) and sample the kept lines inside with their bit set, to
 *       counts[n_loci x samples]; *foreign = 1 when a counted line has a bit
 *       outside allowed[words].  MAGOT_ERR_UNSUPPORTED with
 *       MAGOT_VCF_TOO_MANY_COUNTS in *reason above 2^29 counters.
 *   magot_vcf_time    mean device ms over `iters` runs of: the line index, the
 *       classification, the parse, the runs, the sort, the flags, the counting
 *       pass of the last magot_vcf_count (0 before one), and a device copy of
 *       the text.
 *   magot_vcf_params  rows per piece of the counting pass (longer loci are
 *       counted in pieces combined with atomics), and the limits on samples,
 *       runs and counters.
 * Host side (no device):
 *   magot_vcf_render  the rows "locus,rate,..." joined by LF: per locus with
 *       seqlen >= 1 its text (loci + loci_off[l] .. loci_off[l + 1]) and per
 *       column c of cols str(100.0 * counts[l * n_samples + c] / seqlen) as
 *       Python 2 prints a float.  *text is released with magot_site_text_free.
 */
enum {
  MAGOT_VCF_NO_HEADER = 1,       /* no '#' line that is not "##" */
  MAGOT_VCF_MANY_HEADERS = 2,    /* more than one */
  MAGOT_VCF_HEADER_AFTER_DATA = 3,
  MAGOT_VCF_NO_SAMPLES = 4,      /* the '#' line has fewer than 10 fields */
  MAGOT_VCF_TOO_MANY_SAMPLES = 5,/* more than 1024: the parse kernel's LDS */
  MAGOT_VCF_NO_DATA = 6,
  MAGOT_VCF_FIELD_COUNT = 7,     /* a data line without exactly 9 + S fields */
  MAGOT_VCF_CHROM_FORM = 8,      /* CHROM holds "<:>" */
  MAGOT_VCF_POS_FORM = 9,        /* POS is not digits alone without a leading zero */
  MAGOT_VCF_POS_RANGE = 10,      /* more than 10 digits, or above 2^31 - 1 */
  MAGOT_VCF_NO_GT = 11,          /* FORMAT without GT */
  MAGOT_VCF_EMPTY_GT = 12,       /* a sample column without a GT subfield, or an empty one */
  MAGOT_VCF_EQUALS_FIXED = 13,   /* a sample column equal to one of fields 0-8 */
  MAGOT_VCF_TOO_LARGE = 14,      /* the text is longer than max_bytes */
  MAGOT_VCF_TOO_MANY_LINES = 15, /* more than 2^31 - 1 lines: 32-bit line numbers */
  MAGOT_VCF_TOO_MANY_RUNS = 16,  /* more than 2^20 CHROM runs: the host names each */
  MAGOT_VCF_LINE_TOO_LONG = 17,  /* 2^31 bytes or more: 32-bit field starts */
  MAGOT_VCF_TOO_MANY_COUNTS = 18,/* loci x samples above 2^29: 2 GiB of counters */
  MAGOT_VCF_CARRIAGE_RETURN = 19 /* a CR anywhere: read_vcf drops every CR before it splits */
};
typedef struct magot_vcf magot_vcf;
int magot_vcf_parse(magot_ctx* ctx, const char* text, uint64_t len, uint64_t max_bytes,
                    uint32_t max_samples, uint32_t max_runs, magot_vcf** out, uint32_t* reason,
                    uint64_t* line);
int magot_vcf_sizes(const magot_vcf* p, uint64_t* n_lines, uint64_t* n_data, uint64_t* n_hdr,
                    uint32_t* n_samples, uint32_t* words, uint64_t* n_runs, uint64_t* head_off,
                    uint64_t* head_len);
double magot_vcf_upload_ms(const magot_vcf* p);
int magot_vcf_header_lines(magot_ctx* ctx, magot_vcf* p, uint64_t* off, uint64_t* len);
int magot_vcf_runs(magot_ctx* ctx, magot_vcf* p, uint64_t* off, uint64_t* len);
int magot_vcf_resolve(magot_ctx* ctx, magot_vcf* p, const uint32_t* contig, uint64_t n_runs);
int magot_vcf_tables(magot_ctx* ctx, magot_vcf* p, uint32_t* line, int32_t* pos, uint64_t* hash,
                     uint8_t* kept, uint8_t* first, uint32_t* bits);
int magot_vcf_last_of(magot_ctx* ctx, magot_vcf* p, uint64_t d, uint64_t* line, uint64_t* off,
                      uint64_t* len);
int magot_vcf_count(magot_ctx* ctx, magot_vcf* p, const uint32_t* contig, const uint32_t* lo,
                    const uint32_t* hi, uint64_t n_loci, const uint32_t* allowed, uint32_t* counts,
                    uint32_t* foreign, uint32_t* reason);
int magot_vcf_time(magot_ctx* ctx, magot_vcf* p, int iters, double* ms8, uint64_t* text_bytes);
void magot_vcf_params(uint32_t* split_rows, uint32_t* max_samples, uint32_t* max_runs,
                      uint64_t* max_counts);
void magot_vcf_destroy(magot_vcf* p);
int magot_vcf_render(const char* loci, const uint64_t* loci_off, const int64_t* seqlen,
                     const uint32_t* counts, uint64_t n_loci, uint32_t n_samples,
                     const uint32_t* cols, uint32_t n_cols, uint32_t n_threads, uint8_t** text,
                     uint64_t* bytes);

/*
 * exclude_from_fasta (genome_tools.py:377-391) and fasta2tab
 * (magot_smallfuncs.py:21-29) on the device: the records of a FASTA text, the
 * dict genome.py:854-877 makes of them, an anti-join of its keys against a list
 * of names, and the text reflowed into one line per record.  The text is
 * resident, as a PSL's.
 *
 * A line ends at LF only; the last one may lack it.  A line whose first byte is
 * '>' is a header and opens a record; its name is the rest of the line less the
 * LF and a CR before it.  Every other line adds its bytes, less the LF and a CR
 * before it, to the record's sequence.  A line's cost does not depend on its
 * length.  A name's first word is what Python 2's str.split gives first
 * (blanks: space, TAB, LF, VT, FF, CR).  Only records with a sequence enter the
 * dict: a key's place is that of its first such record, its sequence that of
 * its last.
 *   magot_fastarec_parse  uploads and indexes the text, tables its lines and
 *       records and groups the records by name.  Declined with
 *       MAGOT_ERR_UNSUPPORTED, *out = NULL, *reason a MAGOT_FASTAREC_* code and
 *       *line the 1-based line (0 for the whole-text reasons), in this order: a
 *       text longer than max_bytes (0: a quarter of the free device memory),
 *       before anything of that size is allocated or read; a first byte that is
 *       not '>' (line 1); more than 2^31 - 1 lines; the first line with a CR
 *       that is neither before an LF nor the text's last byte, or with a name
 *       longer than max_name bytes (on one line: the CR); two different keys in
 *       one bucket of the low hash_bits bits (1..64) of CPython 2.7's string
 *       hash (the lowest line that differs from its predecessor in the sorted
 *       order).  A null text with len > 0 and hash_bits outside 1..64 are
 *       MAGOT_ERR_ARG before any launch.
 *   magot_fastarec_sizes  lines, records, records with a sequence, keys.
 *   magot_fastarec_upload_ms  as magot_psl_upload_ms.
 *   magot_fastarec_records  per record in file order: its header's 0-based
 *       line, the name's offset and length, the sequence length, the name's
 *       hash; the first word's offset, length and hash, and 1 where the name
 *       has no word (then the word is empty, at the name's start).  Any pointer
 *       may be NULL.
 *   magot_fastarec_keys  per key in first-seen order: the hash, the first and
 *       the last record with a sequence, and the first record's no-word flag.
 *   magot_fastarec_exclude  keep[k] = 0 where key k -- its first word with
 *       first_word != 0; the empty word where it has none -- equals one of the m
 *       names blob[off[j] .. off[j + 1]); else 1.  Offsets that decrease or leave
 *       the blob (blob_len bytes) are MAGOT_ERR_RANGE before any launch.
 *   magot_fastarec_render  the records rec[0..n) (each below the record count,
 *       else MAGOT_ERR_RANGE before any launch) in that order, into a device
 *       buffer of the handle: style 0 '>' name LF sequence LF; style 1 name TAB
 *       sequence LF, and a lone LF for n = 0.  *bytes: the text's length.
 *   magot_fastarec_render_fetch  that text to the host (cap >= its length).
 *   magot_fastarec_time  mean device ms over `iters` runs of: the line index,
 *       the line table, the names, the sort, the keys, the reflow of every
 *       record in file order in style 1 (*reflow_bytes), and a device copy of
 *       the text (*text_bytes), in ms7[0..6].  The handle's answers stand
 *       afterwards; a rendered text does not.
 *   magot_fastarec_params  the longest name in bytes, the piece of a sequence
 *       line one lane slot of the reflow copies, and the bytes of a text block
 *       of the line index.
 */
enum {
  MAGOT_FASTAREC_LEADING_TEXT = 1,   /* the first byte is not '>' */
  MAGOT_FASTAREC_STRAY_CR = 2,       /* a CR not before an LF and not the last byte */
  MAGOT_FASTAREC_LONG_NAME = 3,      /* a name longer than one lane hashes */
  MAGOT_FASTAREC_HASH_COLLISION = 4, /* two keys in one bucket of the masked hash */
  MAGOT_FASTAREC_TOO_LARGE = 5,      /* the text is longer than max_bytes */
  MAGOT_FASTAREC_TOO_MANY_LINES = 6  /* more than 2^31 - 1 lines */
};
enum { MAGOT_FASTAREC_STYLE_FASTA = 0, MAGOT_FASTAREC_STYLE_TAB = 1 };
typedef struct magot_fastarec magot_fastarec;
int magot_fastarec_parse(magot_ctx* ctx, const char* text, uint64_t len, uint32_t hash_bits,
                         uint64_t max_bytes, magot_fastarec** out, uint32_t* reason,
                         uint64_t* line);
int magot_fastarec_sizes(const magot_fastarec* p, uint64_t* n_lines, uint64_t* n_records,
                         uint64_t* n_with_sequence, uint64_t* n_keys);
double magot_fastarec_upload_ms(const magot_fastarec* p);
int magot_fastarec_records(magot_ctx* ctx, magot_fastarec* p, uint32_t* line, uint64_t* name_off,
                           uint32_t* name_len, uint64_t* seq_len, uint64_t* hash,
                           uint64_t* word_off, uint32_t* word_len, uint64_t* word_hash,
                           uint32_t* no_word);
int magot_fastarec_keys(magot_ctx* ctx, magot_fastarec* p, uint64_t* hash, uint32_t* first_record,
                        uint32_t* last_record, uint32_t* no_word);
int magot_fastarec_exclude(magot_ctx* ctx, magot_fastarec* p, const uint8_t* blob,
                           uint64_t blob_len, const uint64_t* off, uint64_t m, int first_word,
                           uint8_t* keep);
int magot_fastarec_render(magot_ctx* ctx, magot_fastarec* p, const uint32_t* rec, uint64_t n,
                          uint32_t style, uint64_t* bytes);
int magot_fastarec_render_fetch(magot_ctx* ctx, magot_fastarec* p, uint8_t* out, uint64_t cap);
int magot_fastarec_time(magot_ctx* ctx, magot_fastarec* p, int iters, double* ms7,
                        uint64_t* text_bytes, uint64_t* reflow_bytes);
void magot_fastarec_params(uint32_t* max_name, uint32_t* piece, uint32_t* text_block);
void magot_fastarec_destroy(magot_fastarec* p);

/*
 * replace_names (genome_tools.py:431-446) on the device: every occurrence of a
 * key -- a name of the table and the one-byte delimiter d behind it -- in a
 * text replaced by the key's value and d.  The text is resident, as a PSL's.
 *
 * A field is what lies between two ds of a line (lines end at LF).  The device
 * rewrites a field at most once: the suffix of it that is the name of lowest
 * rank among the names that are suffixes of it becomes that name's value.  That
 * is what the reference's loop over all keys prints when no name and no value
 * holds d and no key's value feeds a later key (genome_tools.replace_names
 * checks both; this interface does not).  The table's n_keys names are distinct,
 * each of 1..max_name bytes, name k = names[name_off[k] .. name_off[k + 1]), its
 * value values[val_off[k] .. val_off[k + 1]), rank[k] < n_keys its place in the
 * order the keys are tried.  The output is the rewritten text with its last
 * byte replaced by LF (`print line[:-1]`); an empty text gives an empty one.
 *   magot_rename_parse  uploads text and table, builds the lookup structure
 *       (an open-addressing table keyed by the low hash_bits bits, 1..64, of a
 *       hash of the name from its last byte to its first), finds the field
 *       ends, matches them and lays the output out.  Declined with
 *       MAGOT_ERR_UNSUPPORTED, *out = NULL and *reason a MAGOT_RENAME_* code: a
 *       table of 2^30 names or 4 GiB of names or of values; a text longer than
 *       max_bytes (0: a quarter of the free device memory), before anything of
 *       that size is allocated or read, or one whose field tables exceed half
 *       the free device memory; two names in one bucket of the masked hash
 *       (equal names included).  MAGOT_ERR_ARG before any launch: a null
 *       argument, hash_bits outside 1..64, d above 255 or LF.  MAGOT_ERR_RANGE
 *       before any launch: offsets that do not begin at 0, decrease or leave
 *       their blob (their last entry is the blob's length), a name that is empty
 *       or longer than max_name, a rank of n_keys or more.
 *   magot_rename_sizes  the text's lines, its field ends, the hits, the output's
 *       bytes.
 *   magot_rename_upload_ms  as magot_psl_upload_ms.
 *   magot_rename_hits  per hit in text order: the offset of its d, the key.
 *       Either pointer may be NULL.
 *   magot_rename_render  the output into a device buffer of the handle; *bytes:
 *       its length.
 *   magot_rename_render_fetch  that text to the host (cap >= its length).
 *   magot_rename_time  mean device ms over `iters` runs of: the table build, the
 *       field ends, the match, the layout, the copy into the output
 *       (*out_bytes), and a device copy of the text (*text_bytes), in
 *       ms6[0..5].  The handle's answers stand afterwards; a rendered text does
 *       not.
 *   magot_rename_params  the longest name in bytes, the bytes of a text block
 *       of the field index, and the piece of an unchanged run one lane slot of
 *       the copy takes.
 */
enum {
  MAGOT_RENAME_TOO_LARGE = 1,       /* the text or its field tables */
  MAGOT_RENAME_HASH_COLLISION = 2,  /* two names in one bucket of the masked hash */
  MAGOT_RENAME_TABLE_TOO_LARGE = 3  /* 2^30 names, or 4 GiB of names or values */
};
typedef struct magot_rename magot_rename;
int magot_rename_parse(magot_ctx* ctx, const char* text, uint64_t len, const uint8_t* names,
                       const uint64_t* name_off, const uint8_t* values, const uint64_t* val_off,
                       const uint32_t* rank, uint64_t n_keys, uint32_t delim, uint32_t hash_bits,
                       uint64_t max_bytes, magot_rename** out, uint32_t* reason);
int magot_rename_sizes(const magot_rename* p, uint64_t* n_lines, uint64_t* n_fields,
                       uint64_t* n_hits, uint64_t* out_bytes);
double magot_rename_upload_ms(const magot_rename* p);
int magot_rename_hits(magot_ctx* ctx, magot_rename* p, uint64_t* end, uint32_t* key);
int magot_rename_render(magot_ctx* ctx, magot_rename* p, uint64_t* bytes);
int magot_rename_render_fetch(magot_ctx* ctx, magot_rename* p, uint8_t* out, uint64_t cap);
int magot_rename_time(magot_ctx* ctx, magot_rename* p, int iters, double* ms6,
                      uint64_t* text_bytes, uint64_t* out_bytes);
void magot_rename_params(uint32_t* max_name, uint32_t* text_block, uint32_t* piece);
void magot_rename_destroy(magot_rename* p);

/*
 * Column cuts of a tab-separated text on the device: tab2fasta
 * (magot_smallfuncs.py:12-18) and repeatmasker2augustushints
 * (genome_tools.py:449-454).  The text is resident, as a PSL's.
 *
 * A cut is a program of at most max_items items run on every line (lines end
 * at LF).  A line with fewer than `need` TABs is skipped
 * (MAGOT_TABCUT_SHORT_SKIP) or reported (MAGOT_TABCUT_SHORT_ERROR) and prints
 * nothing; every other line prints its items one after the other.  An item is
 * a literal, the b bytes at offset a of `literals`, or a field range, the
 * source bytes from the first byte of field a to the last byte of field b,
 * the TABs between them included (a <= b <= need; fields count from 0).  A
 * field ends at one of the line's first `need` TABs; field `need` ends at the
 * next TAB when the line has one, else at the line's end less the LF and less
 * one CR before it.  tab2fasta is need 1, MAGOT_TABCUT_SHORT_ERROR, cr_check 1
 * and ">" F[0..0] LF F[1..1] LF; the hints are need 6, MAGOT_TABCUT_SHORT_SKIP,
 * cr_check 0 and F[0..1] "\tnonexonpart\t" F[3..5] "\t.\t.\tpri=2;src=RM\n".
 * No pass reads a field's bytes: a line costs a search in the TAB offsets and
 * its items, whatever its length.
 *   magot_tabcut_parse  uploads text and literals, indexes the LFs and the
 *       TABs, gives every line its verdict and lays the output out.  Declined
 *       with MAGOT_ERR_UNSUPPORTED, *out = NULL and *reason a MAGOT_TABCUT_*
 *       code: a text longer than max_bytes (0: a quarter of the free device
 *       memory), before anything of that size is allocated or read, or one
 *       whose tables exceed half the free device memory; 2^31 - 1 lines or
 *       more; with cr_check, a CR that is neither directly before an LF nor the
 *       text's last byte.  MAGOT_ERR_ARG before any launch: a null argument,
 *       more than max_items items, an item of no known kind, a field range
 *       that decreases or names a field above `need`, a literal that leaves
 *       the blob, a short_mode that is neither of the two.  A short line under
 *       MAGOT_TABCUT_SHORT_ERROR is no decline: the parse succeeds and
 *       magot_tabcut_sizes reports the line.
 *   magot_tabcut_sizes  the text's lines, its TABs, the kept lines, the
 *       output's pieces and bytes, and the lowest short line of error mode
 *       (0-based), all ones when there is none.
 *   magot_tabcut_upload_ms  as magot_psl_upload_ms.
 *   magot_tabcut_rows  per line: its verdict (MAGOT_TABCUT_LINE_*) and where
 *       its output begins.  Either pointer may be NULL.
 *   magot_tabcut_render  the kept lines' output into a device buffer of the
 *       handle; *bytes: its length.
 *   magot_tabcut_render_fetch  that text to the host (cap >= its length).
 *   magot_tabcut_time  mean device ms over `iters` runs of: the two indexes,
 *       the rows, the layout, the piece list, the copy into the output
 *       (*out_bytes), and a device copy of the text (*text_bytes), in
 *       ms6[0..5].  The handle's answers stand afterwards; a rendered text does
 *       not.
 *   magot_tabcut_params  the bytes of an item one lane slot of the copy takes,
 *       the bytes of a text block of the indexes, and the most items of a
 *       program.
 */
enum {
  MAGOT_TABCUT_STRAY_CR = 1,       /* a CR in mid-line (cr_check) */
  MAGOT_TABCUT_TOO_LARGE = 2,      /* the text or its line and TAB tables */
  MAGOT_TABCUT_TOO_MANY_LINES = 3  /* 2^31 - 1 lines or more */
};
enum { MAGOT_TABCUT_ITEM_LITERAL = 0, MAGOT_TABCUT_ITEM_FIELDS = 1 };
enum { MAGOT_TABCUT_SHORT_SKIP = 0, MAGOT_TABCUT_SHORT_ERROR = 1 };
enum { MAGOT_TABCUT_LINE_SKIPPED = 0, MAGOT_TABCUT_LINE_KEPT = 1, MAGOT_TABCUT_LINE_SHORT = 2 };
typedef struct magot_tabcut_item {
  uint32_t kind; /* MAGOT_TABCUT_ITEM_* */
  uint32_t a, b; /* a literal: offset and length in the blob; fields: first and last */
} magot_tabcut_item;
typedef struct magot_tabcut magot_tabcut;
int magot_tabcut_parse(magot_ctx* ctx, const char* text, uint64_t len,
                       const magot_tabcut_item* items, uint32_t n_items, const uint8_t* literals,
                       uint64_t literals_len, uint32_t need, uint32_t short_mode,
                       uint32_t cr_check, uint64_t max_bytes, magot_tabcut** out,
                       uint32_t* reason);
int magot_tabcut_sizes(const magot_tabcut* p, uint64_t* n_lines, uint64_t* n_tabs,
                       uint64_t* n_kept, uint64_t* n_pieces, uint64_t* out_bytes,
                       uint64_t* short_line);
double magot_tabcut_upload_ms(const magot_tabcut* p);
int magot_tabcut_rows(magot_ctx* ctx, magot_tabcut* p, uint8_t* verdict, uint64_t* offset);
int magot_tabcut_render(magot_ctx* ctx, magot_tabcut* p, uint64_t* bytes);
int magot_tabcut_render_fetch(magot_ctx* ctx, magot_tabcut* p, uint8_t* out, uint64_t cap);
int magot_tabcut_time(magot_ctx* ctx, magot_tabcut* p, int iters, double* ms6,
                      uint64_t* text_bytes, uint64_t* out_bytes);
void magot_tabcut_params(uint32_t* piece, uint32_t* text_block, uint32_t* max_items);
void magot_tabcut_destroy(magot_tabcut* p);

/*
 * write_gff (genome.py:228-238, 616-645, 733-778) as a table of output lines:
 * the annotation lowered on the host, its text rendered on the device.
 *
 * One magot_gffrow stands for one output line.  `line_off` is the start of a
 * line of the GFF text with at least eight tabs: its columns 1, 2, 3, 6, 7 and
 * 8 are copied or classified from there.  A reference (offset, length) below
 * the text's length points into the text, one at or above it into the blob
 * (offset - text length).  By kind:
 *   MAGOT_GFFROW_LINE         c1 c2 c3 lo hi score c7 phase ID=<id>[;Parent=<parent>]
 *   MAGOT_GFFROW_EXON_TWIN    c1 c2 exon lo hi score c7 phase ID=ExonOf<id>[;Parent=<parent>]
 *   MAGOT_GFFROW_GTF          c1 c2 c3 lo hi score c7 phase transcript_id <id>;gene_id <parent>
 *   MAGOT_GFFROW_MADE_PARENT  c1 . <type> lo hi . c7 . ID=<id>[;Parent=<parent>]
 * joined by tabs and ended by LF; ";Parent=" only with MAGOT_GFFROW_HAS_PARENT.
 * lo and hi print as decimal integers.  score is column 6 as Python 2 prints
 * float(column 6): "." when the column has no ASCII digit and no ASCII letter;
 * the normalised literal (leading zeros dropped, one kept; trailing fraction
 * zeros dropped, ".0" when none remains; the sign kept) when it is -?D+,
 * -?D+.D* or -?.D+ with at most 12 digits from its first to its last non-zero
 * digit, at most 12 integer digits after the leading zeros and, its integer
 * part being zero, at most 3 zeros before the fraction's first non-zero digit;
 * any other column declines the table.  phase is column 8 when it is exactly 0, 1 or 2, else ".".
 *
 *   magot_gff_lower_write  walks a plan read with MAGOT_GFF_FOR_WRITE in
 *       write_gff's order (flags: MAGOT_GFF_ORDER_PY2) for `format`
 *       (MAGOT_GFFFMT_*), any number of times; the rows replace the plan's last
 *       ones, the blob is the reader's (made-up names, then every table's name)
 *       and the same for every lowering.  MAGOT_ERR_UNSUPPORTED where the reference raises or
 *       where a row cannot say what it prints: a parent without children, a gtf
 *       line without parent or grandparent, an attribute that shadows a name
 *       get_gff reads, a CR in the first eight columns, an exon twin whose
 *       whole-line replaces would touch more than the type and the leading
 *       "ID=".
 *   magot_gffplan_write_views  the rows and the blob of the last lowering (the
 *       plan's memory).
 *   magot_gffwrite_open  text, blob and rows (any caller's) made resident, every
 *       row sized and the output laid out.  MAGOT_ERR_RANGE before any launch: a
 *       line_off beyond the text, a reference that leaves text and blob, a kind
 *       that is none of the four; MAGOT_ERR_ARG: a reference of 2^28 bytes or
 *       more.  Declined with MAGOT_ERR_UNSUPPORTED, *out = NULL, *reason a
 *       MAGOT_GFFWRITE_* code and *row the first offending row (1-based).
 *   magot_gffwrite_sizes  the rows and the output's bytes.
 *   magot_gffwrite_render  the text into a device buffer of the handle.
 *   magot_gffwrite_render_fetch  that text to the host (cap >= its length).
 *   magot_gffwrite_time  mean device ms over `iters` runs of: the sizes, the
 *       scan, the render (*out_bytes) and a device copy of as many bytes, in
 *       ms4[0..3].
 *   magot_gffwrite_params  the rows one wave renders, the threads of a
 *       workgroup, and the bytes within which a line's eighth tab must lie.
 */
typedef struct magot_gffrow {
  uint64_t line_off;   /* the source line's first byte */
  int64_t lo, hi;
  uint64_t id_off;     /* ID; under gtf the parent (transcript_id) */
  uint64_t parent_off; /* parent; under gtf the grandparent (gene_id) */
  uint64_t type_off;   /* MAGOT_GFFROW_MADE_PARENT: the type's name */
  uint32_t id_len, parent_len;
  uint32_t type_len;
  uint32_t kind;       /* MAGOT_GFFROW_* | MAGOT_GFFROW_HAS_PARENT */
} magot_gffrow;
enum {
  MAGOT_GFFROW_LINE = 0,
  MAGOT_GFFROW_EXON_TWIN = 1,
  MAGOT_GFFROW_GTF = 2,
  MAGOT_GFFROW_MADE_PARENT = 3
};
#define MAGOT_GFFROW_HAS_PARENT 0x100u
enum { MAGOT_GFFFMT_GFF3 = 0, MAGOT_GFFFMT_GTF = 1, MAGOT_GFFFMT_EXON_ADDED = 2 };
enum {
  MAGOT_GFFWRITE_TOO_LARGE = 1, /* text, blob and rows against max_bytes */
  MAGOT_GFFWRITE_SCORE = 2,     /* a score outside the two classes */
  MAGOT_GFFWRITE_COLUMNS = 3    /* no eighth tab within the line's first max_head bytes */
};
int magot_gff_lower_write(magot_gffplan* p, uint32_t format, uint32_t flags, uint64_t* n_rows,
                          uint64_t* blob_len);
int magot_gffplan_write_views(const magot_gffplan* p, const magot_gffrow** rows, uint64_t* n_rows,
                              const uint8_t** blob, uint64_t* blob_len);
typedef struct magot_gffwrite magot_gffwrite;
int magot_gffwrite_open(magot_ctx* ctx, const char* text, uint64_t len, const uint8_t* blob,
                        uint64_t blob_len, const magot_gffrow* rows, uint64_t n_rows,
                        uint64_t max_bytes, magot_gffwrite** out, uint32_t* reason, uint64_t* row);
int magot_gffwrite_sizes(const magot_gffwrite* p, uint64_t* n_rows, uint64_t* out_bytes);
double magot_gffwrite_upload_ms(const magot_gffwrite* p);
int magot_gffwrite_render(magot_ctx* ctx, magot_gffwrite* p, uint64_t* bytes);
int magot_gffwrite_render_fetch(magot_ctx* ctx, magot_gffwrite* p, uint8_t* out, uint64_t cap);
int magot_gffwrite_time(magot_ctx* ctx, magot_gffwrite* p, int iters, double* ms4,
                        uint64_t* text_bytes, uint64_t* out_bytes);
void magot_gffwrite_params(uint32_t* rows_per_group, uint32_t* threads, uint32_t* max_head);
void magot_gffwrite_destroy(magot_gffwrite* p);

#ifdef __cplusplus
}
#endif
#endif /* MAGOT_H */
