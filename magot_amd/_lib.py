"""ctypes binding of libmagot.so (C ABI: include/magot.h).

The library is loaded from the package directory (built in-tree by
``magot_amd.build``).  There is no fallback: if the library is missing, or no
HIP device is visible when a device call is made, a ``MagotError`` is raised.
"""

import ctypes
import os
import threading

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
# MAGOT_LIB: an alternative build of the same library (A/B kernel experiments)
LIB_PATH = os.environ.get('MAGOT_LIB') or os.path.join(HERE, 'libmagot.so')

OUT_NUC = 1
OUT_PEP = 2
OUT_GENOME_ORDER = 4  # layout flag: records in genome order in the device buffers

EXON_DTYPE = np.dtype([('start_rc', '<u8'), ('contig', '<u4'), ('len', '<u4')])
TX_DTYPE = np.dtype([('exon_begin', '<u8'), ('n_exons', '<u4'), ('flags', '<u4')])
RC_BIT = np.uint64(1 << 63)

# Every symbol include/magot.h declares (checked by tests/test_abi.py).
EXPORTS = (
    'magot_abi_version', 'magot_last_error', 'magot_device_count',
    'magot_ctx_create', 'magot_ctx_destroy', 'magot_ctx_sync', 'magot_ctx_info',
    'magot_genome_load', 'magot_genome_stats', 'magot_genome_destroy',
    'magot_plan_create', 'magot_plan_destroy', 'magot_plan_execute', 'magot_plan_fetch',
    'magot_run', 'magot_plan_time', 'magot_plan_time_b2b', 'magot_plan_device_outputs',
    'magot_plan_layout',
    'magot_plan_algorithmic_bytes',
    'magot_revcomp_batch', 'magot_translate_sizes', 'magot_translate_batch',
    'magot_codon_symbols', 'magot_revcomp', 'magot_translate',
    'magot_gff_plan', 'magot_gff_read', 'magot_gff_lower', 'magot_flank_plan',
    'magot_gffplan_tables', 'magot_gffplan_table_views', 'magot_gffplan_render',
    'magot_gffplan_destroy',
    'magot_gffplan_selections', 'magot_cds_scan', 'magot_cds_render',
    'magot_genome_export', 'magot_genome_copy_arena', 'magot_genome_attach',
    'magot_plan_copy_outputs',
    'magot_orf6_sizes', 'magot_orf6_batch', 'magot_plan_orf6', 'magot_orf6_execute',
    'magot_orf6_fetch', 'magot_orf6_time', 'magot_orf6_time_b2b', 'magot_orf6_destroy',
    'magot_genome_load_fasta', 'magot_genome_contigs', 'magot_fasta_read',
    'magot_fasta_text_create', 'magot_fasta_text_execute', 'magot_fasta_text_fetch',
    'magot_fasta_text_time', 'magot_fasta_text_destroy',
    'magot_genome_load_ex', 'magot_genome_wire_ranges', 'magot_genome_attach_wire',
    'magot_copy_segments', 'magot_ctx_mark', 'magot_ctx_elapsed', 'magot_orf6_copy_outputs',
    'magot_genome_wire_export', 'magot_genome_wire_import',
    'magot_debug_tile_blocks', 'magot_debug_tile_cut', 'magot_debug_plan',
    'magot_debug_text_index', 'magot_debug_text_lines', 'magot_debug_piece_copy',
    'magot_debug_text_assembly', 'magot_debug_orf6_tiles', 'magot_debug_orf6_batch',
    'magot_orf6_poison',
    'magot_orfcall_tile', 'magot_orfcall_create', 'magot_orfcall_fetch', 'magot_orfcall_text',
    'magot_orfcall_text_fetch', 'magot_orfcall_time', 'magot_orfcall_destroy',
    'magot_mask_piece', 'magot_mask_plan', 'magot_maskplan_table', 'magot_maskplan_destroy',
    'magot_mask_fasta_check', 'magot_mask_create', 'magot_mask_execute', 'magot_mask_fetch',
    'magot_mask_coverage_fetch', 'magot_mask_time', 'magot_mask_destroy',
    'magot_track_rank_block', 'magot_track_create', 'magot_track_base_class', 'magot_track_paint',
    'magot_track_set_bytes', 'magot_track_get_bytes', 'magot_track_fetch',
    'magot_track_windows_create', 'magot_track_windows_fetch', 'magot_track_transitions',
    'magot_track_transitions_fetch', 'magot_track_count', 'magot_track_time',
    'magot_track_windows_destroy', 'magot_track_destroy',
    'magot_depth_block', 'magot_depth_parse', 'magot_depth_runs', 'magot_depth_values',
    'magot_depth_sums', 'magot_depth_time', 'magot_depth_destroy',
    'magot_fq_dense', 'magot_fq_parse', 'magot_fq_stats', 'magot_fq_histogram', 'magot_fq_time',
    'magot_fq_destroy',
    'magot_overlap_coord_range', 'magot_overlap_lane_scan', 'magot_overlap_create',
    'magot_overlap_purge', 'magot_overlap_counts', 'magot_overlap_time', 'magot_overlap_destroy',
    'magot_overlap_plan', 'magot_ovplan_table', 'magot_ovplan_render', 'magot_ovplan_destroy',
    'magot_psl_parse', 'magot_psl_sizes', 'magot_psl_upload_ms', 'magot_psl_pass_lines',
    'magot_psl_groups', 'magot_psl_time', 'magot_psl_destroy', 'magot_psl_order',
    'magot_psl_render',
    'magot_site_create', 'magot_site_execute', 'magot_site_counts', 'magot_site_time',
    'magot_site_params', 'magot_site_destroy', 'magot_site_render', 'magot_site_text_free',
    'magot_vcf_parse', 'magot_vcf_sizes', 'magot_vcf_upload_ms', 'magot_vcf_header_lines',
    'magot_vcf_runs', 'magot_vcf_resolve', 'magot_vcf_tables', 'magot_vcf_last_of',
    'magot_vcf_count', 'magot_vcf_time', 'magot_vcf_params', 'magot_vcf_destroy',
    'magot_vcf_render',
    'magot_fastarec_parse', 'magot_fastarec_sizes', 'magot_fastarec_upload_ms',
    'magot_fastarec_records', 'magot_fastarec_keys', 'magot_fastarec_exclude',
    'magot_fastarec_render', 'magot_fastarec_render_fetch', 'magot_fastarec_time',
    'magot_fastarec_params', 'magot_fastarec_destroy',
    'magot_rename_parse', 'magot_rename_sizes', 'magot_rename_upload_ms', 'magot_rename_hits',
    'magot_rename_render', 'magot_rename_render_fetch', 'magot_rename_time',
    'magot_rename_params', 'magot_rename_destroy',
    'magot_tabcut_parse', 'magot_tabcut_sizes', 'magot_tabcut_upload_ms', 'magot_tabcut_rows',
    'magot_tabcut_render', 'magot_tabcut_render_fetch', 'magot_tabcut_time',
    'magot_tabcut_params', 'magot_tabcut_destroy',
    'magot_gff_lower_write', 'magot_gffplan_write_views',
    'magot_gffwrite_open', 'magot_gffwrite_sizes', 'magot_gffwrite_upload_ms',
    'magot_gffwrite_render', 'magot_gffwrite_render_fetch', 'magot_gffwrite_time',
    'magot_gffwrite_params', 'magot_gffwrite_destroy',
    'magot_longorf_create', 'magot_longorf_execute', 'magot_longorf_fetch', 'magot_longorf_text',
    'magot_longorf_text_fetch', 'magot_longorf_time', 'magot_longorf_params',
    'magot_longorf_destroy', 'magot_gff_lower_cds', 'magot_gffplan_cds_views',
)

ERR_ARG = -1
ERR_HIP = -2
ERR_RANGE = -3
ERR_STATE = -4
ERR_UNSUPPORTED = -5
GFF_PROTEIN = 1
GFF_ORDER_PY2 = 2
GFF_LONGEST = 4
GFF_GENOMIC = 8
GFF_FROM_EXONS = 16
GFF_FOR_WRITE = 32
GFF_FORMATS = {'simple gff3': 0, 'gtf': 1, 'exon added gff3': 2}
CDS_NAMES = {'CDS': 0, 'transcript': 1, 'gene': 2}  # magot_gff_lower_cds' names_from
GFFROW_LINE, GFFROW_EXON_TWIN, GFFROW_GTF, GFFROW_MADE_PARENT = 0, 1, 2, 3
GFFROW_HAS_PARENT = 0x100
PACK_HOST = 1
ORF_FROM_ATG = 1
ORF_LONGEST = 2
ORF_REC_NONE = 1
ORF_REC_NO_LONGEST = 2
MASK_HARD = 1
MASK_KEEP_CASE = 2
TRACK_GC = 1
TRACK_REPLACE = 2
# magot_depth_parse's reasons (MAGOT_DEPTH_*), by code
DEPTH_REASONS = (None, 'empty line', 'leading blank', 'byte outside the grammar',
                 'name longer than 255 bytes', 'fewer than three fields', 'sign on a number',
                 'not a number', 'number out of range', 'position out of sequence',
                 'repeated contig', 'line longer than a chunk', 'more than 2^31-1 lines',
                 'too many runs')
OVERLAP_NO_SEQ = 0xffffffff
# magot_overlap_plan's reasons (MAGOT_OVERLAP_*), by code
OVERLAP_REASONS = (None, 'bad integer in the first file', 'bad integer in the second file',
                   'coordinate beyond the key range', 'too many seqids')
# magot_psl_parse's reasons (MAGOT_PSL_*), by code
PSL_REASONS = (None, 'few_fields', 'integer_form', 'number_range', 'hash_collision', 'too_large',
               'too_many_lines')
# magot_vcf_parse's and magot_vcf_count's reasons (MAGOT_VCF_*), by code
VCF_REASONS = (None, 'no_header', 'many_headers', 'header_after_data', 'no_samples',
               'too_many_samples', 'no_data', 'field_count', 'chrom_form', 'pos_form', 'pos_range',
               'no_gt', 'empty_gt', 'equals_fixed', 'too_large', 'too_many_lines', 'too_many_runs',
               'line_too_long', 'too_many_counts', 'carriage_return')
# magot_fastarec_parse's reasons (MAGOT_FASTAREC_*), by code
FASTAREC_REASONS = (None, 'leading_text', 'stray_cr', 'long_name', 'hash_collision', 'too_large',
                    'too_many_lines')
FASTAREC_STYLES = {'fasta': 0, 'tab': 1}
# magot_rename_parse's reasons (MAGOT_RENAME_*), by code
RENAME_REASONS = (None, 'too_large', 'hash_collision', 'table_too_large')
# magot_tabcut_parse's reasons (MAGOT_TABCUT_*), by code
TABCUT_REASONS = (None, 'stray_cr', 'too_large', 'too_many_lines')
TABCUT_LITERAL, TABCUT_FIELDS = 0, 1
TABCUT_SHORT = {'skip': 0, 'error': 1}
TABCUT_SKIPPED, TABCUT_KEPT, TABCUT_SHORT_LINE = 0, 1, 2
# magot_tabcut_item (include/magot.h)
TABCUT_ITEM_DTYPE = np.dtype([('kind', '<u4'), ('a', '<u4'), ('b', '<u4')])
# magot_gffwrite_open's reasons (MAGOT_GFFWRITE_*), by code
GFFWRITE_REASONS = (None, 'too_large', 'score', 'columns')
# magot_gffrow (include/magot.h)
GFFROW_DTYPE = np.dtype([('line_off', '<u8'), ('lo', '<i8'), ('hi', '<i8'), ('id_off', '<u8'),
                         ('parent_off', '<u8'), ('type_off', '<u8'), ('id_len', '<u4'),
                         ('parent_len', '<u4'), ('type_len', '<u4'), ('kind', '<u4')])
MASK_INTERVAL_DTYPE = np.dtype([('contig', '<u4'), ('start', '<u4'), ('len', '<u4')])


class MagotError(RuntimeError):
    """A libmagot call failed (status + magot_last_error text)."""


_u8p = ctypes.POINTER(ctypes.c_uint8)
_u64p = ctypes.POINTER(ctypes.c_uint64)
_i64p = ctypes.POINTER(ctypes.c_int64)
_i32p = ctypes.POINTER(ctypes.c_int32)
_vp = ctypes.c_void_p

_lib = None
_lib_lock = threading.RLock()


def _declare(lib):
    sig = {
        'magot_abi_version': (ctypes.c_int, []),
        'magot_last_error': (ctypes.c_char_p, []),
        'magot_device_count': (ctypes.c_int, []),
        'magot_ctx_create': (ctypes.c_int, [ctypes.c_int, ctypes.POINTER(_vp)]),
        'magot_ctx_destroy': (None, [_vp]),
        'magot_ctx_sync': (ctypes.c_int, [_vp]),
        'magot_ctx_info': (ctypes.c_int, [_vp, ctypes.POINTER(ctypes.c_int),
                                          ctypes.POINTER(ctypes.c_int)]),
        'magot_genome_load': (ctypes.c_int, [_vp, ctypes.POINTER(_u8p), _u64p, ctypes.c_uint32,
                                             ctypes.POINTER(_vp)]),
        'magot_genome_stats': (ctypes.c_int, [_vp, _u64p, _u64p, _u64p]),
        'magot_genome_destroy': (None, [_vp]),
        'magot_plan_create': (ctypes.c_int, [_vp, _vp, _vp, ctypes.c_uint64, _vp, ctypes.c_uint64,
                                             ctypes.c_uint32, ctypes.POINTER(_vp), _u64p, _u64p]),
        'magot_plan_destroy': (None, [_vp]),
        'magot_plan_execute': (ctypes.c_int, [_vp, _vp]),
        'magot_plan_fetch': (ctypes.c_int, [_vp, _vp, _vp, _vp, _vp, _vp]),
        'magot_run': (ctypes.c_int, [_vp, _vp, _vp, _vp, _vp, _vp]),
        'magot_plan_time': (ctypes.c_int, [_vp, _vp, ctypes.c_int,
                                           ctypes.POINTER(ctypes.c_double)]),
        'magot_plan_time_b2b': (ctypes.c_int, [_vp, _vp, ctypes.c_int,
                                               ctypes.POINTER(ctypes.c_double)]),
        'magot_plan_layout': (ctypes.c_int, [_vp, _vp, _vp]),
        'magot_plan_device_outputs': (ctypes.c_int, [_vp, ctypes.POINTER(_vp),
                                                     ctypes.POINTER(_vp)]),
        'magot_plan_algorithmic_bytes': (ctypes.c_uint64, [_vp]),
        'magot_debug_tile_blocks': (ctypes.c_int, [_vp, _vp, _vp, _vp, ctypes.c_uint64,
                                                   ctypes.c_uint32, _vp, ctypes.c_uint64, _vp, _vp,
                                                   _vp, ctypes.c_uint64, _vp, ctypes.c_uint64,
                                                   _vp]),
        'magot_debug_tile_cut': (ctypes.c_int, [_vp, ctypes.c_uint64, _vp, _vp, ctypes.c_uint64,
                                                ctypes.c_uint32, _vp, ctypes.c_uint64, _vp]),
        'magot_debug_plan': (ctypes.c_int, [_vp, _vp, ctypes.c_uint32, _vp, ctypes.c_uint64, _vp,
                                            ctypes.c_uint64, ctypes.c_uint32, _vp, _vp, _vp, _vp,
                                            _vp, _vp, _vp, _vp]),
        'magot_debug_text_index': (ctypes.c_int, [_vp, _vp, ctypes.c_uint64, ctypes.c_uint64,
                                                  ctypes.c_uint32, ctypes.c_int32, _vp, _u64p,
                                                  _u64p]),
        'magot_debug_text_lines': (ctypes.c_int, [_vp, _vp, ctypes.c_uint64, ctypes.c_uint64,
                                                  ctypes.c_int, ctypes.c_uint32, _vp, _u64p,
                                                  _u64p]),
        'magot_debug_piece_copy': (ctypes.c_int, [_vp, _vp, ctypes.c_uint64, _vp, _vp, _vp,
                                                  ctypes.c_uint64, _vp, ctypes.c_uint64]),
        'magot_debug_text_assembly': (ctypes.c_int, [_vp, _vp, ctypes.c_uint64, _vp,
                                                     ctypes.c_uint64, _vp, ctypes.c_uint64, _vp,
                                                     ctypes.c_uint64, ctypes.c_int, _vp,
                                                     ctypes.c_uint64, _u64p]),
        'magot_revcomp_batch': (ctypes.c_int, [_vp, _vp, _vp, ctypes.c_uint64, _vp]),
        'magot_translate_sizes': (ctypes.c_int, [_vp, ctypes.c_uint64, _vp, _vp, _vp]),
        'magot_translate_batch': (ctypes.c_int, [_vp, _vp, _vp, ctypes.c_uint64, _vp, _vp, _vp,
                                                 _vp, _vp]),
        'magot_codon_symbols': (ctypes.c_int, [_vp, _vp, ctypes.c_uint64, _vp, ctypes.c_uint32,
                                               _vp, _vp]),
        'magot_revcomp': (ctypes.c_int, [_vp, _vp, ctypes.c_uint64, _vp]),
        'magot_translate': (ctypes.c_int, [_vp, _vp, ctypes.c_uint64, ctypes.c_int, ctypes.c_int,
                                           ctypes.c_int, _vp, _i64p]),
        'magot_gff_plan': (ctypes.c_int, [_vp, ctypes.c_uint64,
                                          ctypes.POINTER(ctypes.c_char_p), _u64p, ctypes.c_uint32,
                                          ctypes.c_char_p, ctypes.c_uint32, ctypes.POINTER(_vp),
                                          _u64p, _u64p]),
        'magot_gff_read': (ctypes.c_int, [_vp, ctypes.c_uint64, ctypes.c_uint32,
                                          ctypes.POINTER(_vp)]),
        'magot_gff_lower': (ctypes.c_int, [_vp, ctypes.POINTER(ctypes.c_char_p), _u64p,
                                           ctypes.c_uint32, ctypes.c_char_p, ctypes.c_uint32,
                                           _u64p, _u64p]),
        'magot_flank_plan': (ctypes.c_int, [_vp, ctypes.c_uint64,
                                            ctypes.POINTER(ctypes.c_char_p), _u64p,
                                            ctypes.c_uint32, ctypes.c_char_p, ctypes.c_char_p,
                                            ctypes.c_char_p, ctypes.c_char_p, ctypes.POINTER(_vp),
                                            _u64p, _u64p]),
        'magot_gffplan_tables': (ctypes.c_int, [_vp, _vp, _vp]),
        'magot_gffplan_table_views': (ctypes.c_int, [_vp, ctypes.POINTER(_vp),
                                                     ctypes.POINTER(_vp)]),
        'magot_gffplan_render': (ctypes.c_int, [_vp, _vp, _vp, _vp, _vp, _vp, ctypes.c_uint64,
                                                _u64p]),
        'magot_gffplan_destroy': (None, [_vp]),
        'magot_gffplan_selections': (ctypes.c_int, [_vp, _u64p]),
        'magot_cds_scan': (ctypes.c_int, [_vp, ctypes.c_uint64, _u64p, _u64p, _vp, _vp, _vp, _vp,
                                          ctypes.c_uint64]),
        'magot_cds_render': (ctypes.c_int, [_vp, ctypes.c_uint64, _vp, _vp, _vp, _vp, _vp, _vp,
                                            _vp, ctypes.c_uint64, _u64p]),
        'magot_genome_export': (ctypes.c_int, [_vp, _vp, ctypes.c_uint64, _u64p, _u64p]),
        'magot_genome_copy_arena': (ctypes.c_int, [_vp, _vp]),
        'magot_genome_attach': (ctypes.c_int, [_vp, _vp, ctypes.c_uint64, _vp,
                                               ctypes.POINTER(_vp)]),
        'magot_plan_copy_outputs': (ctypes.c_int, [_vp, _vp, _vp, _vp]),
        'magot_orf6_sizes': (ctypes.c_int, [_vp, ctypes.c_uint64, _vp, _vp, _vp]),
        'magot_orf6_batch': (ctypes.c_int, [_vp, _vp, _vp, ctypes.c_uint64, _vp, _vp, _vp]),
        'magot_debug_orf6_batch': (ctypes.c_int, [_vp, _vp, _vp, ctypes.c_uint64, _vp, _vp, _vp,
                                                  ctypes.c_int32]),
        'magot_debug_orf6_tiles': (ctypes.c_int, [_vp, ctypes.c_uint64, _vp, ctypes.c_uint64, _vp,
                                                  _vp, _vp, _vp, ctypes.c_uint64, _u64p]),
        'magot_orf6_poison': (ctypes.c_int, [_vp, _vp, ctypes.c_uint8]),
        'magot_plan_orf6': (ctypes.c_int, [_vp, _vp, _vp, ctypes.POINTER(_vp), _u64p]),
        'magot_orf6_execute': (ctypes.c_int, [_vp, _vp]),
        'magot_orf6_fetch': (ctypes.c_int, [_vp, _vp, _vp, _vp, _vp]),
        'magot_orf6_time': (ctypes.c_int, [_vp, _vp, ctypes.c_int,
                                           ctypes.POINTER(ctypes.c_double)]),
        'magot_orf6_time_b2b': (ctypes.c_int, [_vp, _vp, ctypes.c_int,
                                               ctypes.POINTER(ctypes.c_double)]),
        'magot_orf6_destroy': (None, [_vp]),
        'magot_fasta_text_create': (ctypes.c_int, [_vp, _vp, _vp, ctypes.POINTER(_vp), _u64p]),
        'magot_fasta_text_execute': (ctypes.c_int, [_vp, _vp]),
        'magot_fasta_text_fetch': (ctypes.c_int, [_vp, _vp, _vp, ctypes.c_uint64, _u64p]),
        'magot_fasta_text_time': (ctypes.c_int, [_vp, _vp, ctypes.c_int,
                                                 ctypes.POINTER(ctypes.c_double)]),
        'magot_fasta_text_destroy': (None, [_vp]),
        'magot_genome_load_fasta': (ctypes.c_int, [_vp, _vp, ctypes.c_uint64,
                                                   ctypes.c_int, ctypes.POINTER(_vp)]),
        'magot_genome_contigs': (ctypes.c_int, [_vp, ctypes.POINTER(ctypes.c_uint32), _vp, _vp,
                                                ctypes.c_uint64, _u64p]),
        'magot_genome_load_ex': (ctypes.c_int, [_vp, ctypes.POINTER(_u8p), _u64p, ctypes.c_uint32,
                                                ctypes.c_uint32, ctypes.POINTER(_vp)]),
        'magot_genome_wire_ranges': (ctypes.c_int, [_vp, _u64p, _u64p,
                                                    ctypes.POINTER(ctypes.c_uint32)]),
        'magot_genome_attach_wire': (ctypes.c_int, [_vp, _vp, ctypes.c_uint64, _vp,
                                                    ctypes.POINTER(_vp)]),
        'magot_genome_wire_export': (ctypes.c_int, [_vp, _vp, ctypes.c_uint64, _u64p]),
        'magot_genome_wire_import': (ctypes.c_int, [_vp, _vp, ctypes.c_uint64, _vp,
                                                    ctypes.c_uint64, ctypes.POINTER(_vp)]),
        'magot_copy_segments': (ctypes.c_int, [_vp, _vp, ctypes.c_uint64, _vp, _vp, _vp,
                                               ctypes.c_uint64]),
        'magot_ctx_mark': (ctypes.c_int, [_vp, ctypes.c_int]),
        'magot_orf6_copy_outputs': (ctypes.c_int, [_vp, _vp, _vp]),
        'magot_ctx_elapsed': (ctypes.c_int, [_vp, ctypes.POINTER(ctypes.c_double)]),
        'magot_fasta_read': (ctypes.c_int, [_vp, ctypes.c_uint64, ctypes.c_int,
                                            ctypes.POINTER(ctypes.c_uint32), _vp, _vp,
                                            ctypes.c_uint64, _u64p, _vp, ctypes.c_uint64]),
        'magot_orfcall_tile': (ctypes.c_uint32, []),
        'magot_orfcall_create': (ctypes.c_int, [_vp, _vp, ctypes.c_uint32, ctypes.POINTER(_vp),
                                                _u64p, _u64p]),
        'magot_orfcall_fetch': (ctypes.c_int, [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
        'magot_orfcall_text': (ctypes.c_int, [_vp, _vp, _vp, _vp, _u64p]),
        'magot_orfcall_text_fetch': (ctypes.c_int, [_vp, _vp, _vp, ctypes.c_uint64]),
        'magot_orfcall_time': (ctypes.c_int, [_vp, _vp, ctypes.c_int, ctypes.c_int,
                                              ctypes.POINTER(ctypes.c_double)]),
        'magot_orfcall_destroy': (None, [_vp]),
        'magot_longorf_create': (ctypes.c_int, [_vp, _vp, _vp, ctypes.POINTER(_vp)]),
        'magot_longorf_execute': (ctypes.c_int, [_vp, _vp, _u64p]),
        'magot_longorf_fetch': (ctypes.c_int, [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
        'magot_longorf_text': (ctypes.c_int, [_vp, _vp, _vp, _vp, ctypes.c_uint64, _u64p]),
        'magot_longorf_text_fetch': (ctypes.c_int, [_vp, _vp, _vp, ctypes.c_uint64]),
        'magot_longorf_time': (ctypes.c_int, [_vp, _vp, ctypes.c_int, ctypes.c_int,
                                              ctypes.POINTER(ctypes.c_double)]),
        'magot_longorf_params': (ctypes.c_int, [_vp, _vp, ctypes.POINTER(ctypes.c_uint32), _u64p]),
        'magot_longorf_destroy': (None, [_vp]),
        'magot_gff_lower_cds': (ctypes.c_int, [_vp, ctypes.POINTER(ctypes.c_char_p), _u64p,
                                               ctypes.c_uint32, ctypes.POINTER(ctypes.c_char_p),
                                               ctypes.c_uint32, _i64p, ctypes.c_uint32,
                                               ctypes.c_uint32, _u64p, _u64p]),
        'magot_gffplan_cds_views': (ctypes.c_int, [_vp, ctypes.POINTER(_vp), ctypes.POINTER(_vp),
                                                   ctypes.POINTER(_vp)]),
        'magot_mask_piece': (ctypes.c_uint32, []),
        'magot_mask_plan': (ctypes.c_int, [_vp, ctypes.c_uint64, ctypes.POINTER(ctypes.c_char_p),
                                           _u64p, ctypes.c_uint32, ctypes.c_char_p,
                                           ctypes.c_uint32, ctypes.POINTER(_vp), _u64p]),
        'magot_maskplan_table': (ctypes.c_int, [_vp, ctypes.POINTER(_vp), _u64p,
                                                ctypes.POINTER(ctypes.c_uint32)]),
        'magot_maskplan_destroy': (None, [_vp]),
        'magot_mask_fasta_check': (ctypes.c_int, [_vp, ctypes.c_uint64, ctypes.c_uint32]),
        'magot_mask_create': (ctypes.c_int, [_vp, _vp, _vp, _vp, _vp, _vp, ctypes.POINTER(_vp),
                                             _u64p]),
        'magot_mask_execute': (ctypes.c_int, [_vp, _vp]),
        'magot_mask_fetch': (ctypes.c_int, [_vp, _vp, _vp, ctypes.c_uint64]),
        'magot_mask_coverage_fetch': (ctypes.c_int, [_vp, _vp, _vp, ctypes.c_uint64, _u64p]),
        'magot_mask_time': (ctypes.c_int, [_vp, _vp, ctypes.c_int,
                                           ctypes.POINTER(ctypes.c_double),
                                           ctypes.POINTER(ctypes.c_double)]),
        'magot_mask_destroy': (None, [_vp]),
        'magot_track_rank_block': (ctypes.c_uint32, []),
        'magot_track_create': (ctypes.c_int, [_vp, _vp, ctypes.POINTER(_vp), _u64p]),
        'magot_track_base_class': (ctypes.c_int, [_vp, _vp, _vp, ctypes.c_uint32]),
        'magot_track_paint': (ctypes.c_int, [_vp, _vp, _vp, ctypes.c_uint64, ctypes.c_int]),
        'magot_track_set_bytes': (ctypes.c_int, [_vp, _vp, ctypes.c_uint32, _vp,
                                                 ctypes.c_uint64]),
        'magot_track_get_bytes': (ctypes.c_int, [_vp, _vp, ctypes.c_uint32, _vp,
                                                 ctypes.c_uint64]),
        'magot_track_fetch': (ctypes.c_int, [_vp, _vp, _vp, ctypes.c_uint64, _u64p]),
        'magot_track_windows_create': (ctypes.c_int, [_vp, _vp, ctypes.c_uint64, ctypes.c_uint64,
                                                      _vp, ctypes.POINTER(_vp), _u64p, _vp]),
        'magot_track_windows_fetch': (ctypes.c_int, [_vp, _vp, _vp, ctypes.c_uint64]),
        'magot_track_transitions': (ctypes.c_int, [_vp, _vp, ctypes.c_uint32, _u64p]),
        'magot_track_transitions_fetch': (ctypes.c_int, [_vp, _vp, _vp, ctypes.c_uint64]),
        'magot_track_count': (ctypes.c_int, [_vp, _vp, _vp, ctypes.c_uint64, _vp]),
        'magot_track_time': (ctypes.c_int, [_vp, _vp, _vp, ctypes.c_uint32, ctypes.c_int, _vp]),
        'magot_track_windows_destroy': (None, [_vp]),
        'magot_track_destroy': (None, [_vp]),
        'magot_depth_block': (ctypes.c_uint32, []),
        'magot_depth_parse': (ctypes.c_int, [_vp, _vp, ctypes.c_uint64, ctypes.c_uint64,
                                             ctypes.c_uint32, ctypes.POINTER(_vp), _u64p, _u64p,
                                             ctypes.POINTER(ctypes.c_uint32), _u64p]),
        'magot_depth_runs': (ctypes.c_int, [_vp, _vp, _vp, _vp, ctypes.c_uint64]),
        'magot_depth_values': (ctypes.c_int, [_vp, _vp, ctypes.c_uint64, ctypes.c_uint64, _vp]),
        'magot_depth_sums': (ctypes.c_int, [_vp, _vp, _vp, _vp, ctypes.c_uint64, _vp,
                                            ctypes.c_uint64, _vp, _vp]),
        'magot_depth_time': (ctypes.c_int, [_vp, _vp, ctypes.c_int, _vp, _u64p]),
        'magot_depth_destroy': (None, [_vp]),
        'magot_fq_dense': (ctypes.c_uint64, []),
        'magot_fq_parse': (ctypes.c_int, [_vp, _vp, ctypes.c_uint64, ctypes.c_uint64,
                                          ctypes.POINTER(_vp)]),
        'magot_fq_stats': (ctypes.c_int, [_vp, _vp, ctypes.POINTER(ctypes.c_uint32)]),
        'magot_fq_histogram': (ctypes.c_int, [_vp, _vp, _vp, _vp, ctypes.c_uint64, _u64p]),
        'magot_fq_time': (ctypes.c_int, [_vp, _vp, ctypes.c_int, _vp, _u64p]),
        'magot_fq_destroy': (None, [_vp]),
        'magot_overlap_coord_range': (None, [_i64p, _i64p]),
        'magot_overlap_lane_scan': (ctypes.c_uint32, []),
        'magot_overlap_create': (ctypes.c_int, [_vp, _vp, _vp, _vp, ctypes.c_uint64,
                                                ctypes.c_uint32, ctypes.POINTER(_vp)]),
        'magot_overlap_purge': (ctypes.c_int, [_vp, _vp, _vp, _vp, _vp, ctypes.c_uint64, _vp]),
        'magot_overlap_counts': (ctypes.c_int, [_vp, _vp, _vp, _vp, _vp, ctypes.c_uint64, _vp]),
        'magot_overlap_time': (ctypes.c_int, [_vp, _vp, ctypes.c_int, _vp, _u64p]),
        'magot_overlap_destroy': (None, [_vp]),
        'magot_overlap_plan': (ctypes.c_int, [_vp, ctypes.c_uint64, _vp, ctypes.c_uint64,
                                              ctypes.POINTER(_vp),
                                              ctypes.POINTER(ctypes.c_uint32)]),
        'magot_ovplan_table': (ctypes.c_int, [_vp, ctypes.c_int, _u64p,
                                              ctypes.POINTER(ctypes.c_uint32)] +
                               [ctypes.POINTER(_vp)] * 6),
        'magot_ovplan_render': (ctypes.c_int, [_vp, _vp, ctypes.c_uint64, _vp, _vp,
                                               ctypes.c_uint64, _u64p]),
        'magot_ovplan_destroy': (None, [_vp]),
        'magot_psl_parse': (ctypes.c_int, [_vp, _vp, ctypes.c_uint64, ctypes.c_uint32,
                                           ctypes.c_uint64, ctypes.POINTER(_vp),
                                           ctypes.POINTER(ctypes.c_uint32), _u64p]),
        'magot_psl_sizes': (ctypes.c_int, [_vp, _u64p, _u64p, _u64p, _u64p]),
        'magot_psl_upload_ms': (ctypes.c_double, [_vp]),
        'magot_psl_pass_lines': (ctypes.c_int, [_vp, _vp, _vp, _vp]),
        'magot_psl_groups': (ctypes.c_int, [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
        'magot_psl_time': (ctypes.c_int, [_vp, _vp, ctypes.c_int, _vp, _u64p]),
        'magot_psl_destroy': (None, [_vp]),
        'magot_psl_order': (ctypes.c_int, [_vp, ctypes.c_uint64, _vp]),
        'magot_psl_render': (ctypes.c_int, [_vp, ctypes.c_uint64, _vp, _vp, ctypes.c_uint64,
                                            ctypes.c_int, _vp, ctypes.c_uint64, _u64p]),
        'magot_site_create': (ctypes.c_int, [_vp, _vp, _vp, _vp, ctypes.c_uint64, ctypes.c_uint64,
                                             ctypes.POINTER(_vp)]),
        'magot_site_execute': (ctypes.c_int, [_vp, _vp]),
        'magot_site_counts': (ctypes.c_int, [_vp, _vp, _vp]),
        'magot_site_time': (ctypes.c_int, [_vp, _vp, ctypes.c_int, ctypes.POINTER(ctypes.c_double)]),
        'magot_site_params': (None, [ctypes.POINTER(ctypes.c_uint32)] * 5),
        'magot_site_destroy': (None, [_vp]),
        'magot_site_render': (ctypes.c_int, [_vp, ctypes.c_uint64, ctypes.c_uint32,
                                             ctypes.POINTER(_vp), _u64p, _u64p]),
        'magot_site_text_free': (None, [_vp]),
        'magot_vcf_parse': (ctypes.c_int, [_vp, _vp, ctypes.c_uint64, ctypes.c_uint64,
                                           ctypes.c_uint32, ctypes.c_uint32, ctypes.POINTER(_vp),
                                           ctypes.POINTER(ctypes.c_uint32), _u64p]),
        'magot_vcf_sizes': (ctypes.c_int, [_vp, _u64p, _u64p, _u64p,
                                           ctypes.POINTER(ctypes.c_uint32),
                                           ctypes.POINTER(ctypes.c_uint32), _u64p, _u64p, _u64p]),
        'magot_vcf_upload_ms': (ctypes.c_double, [_vp]),
        'magot_vcf_header_lines': (ctypes.c_int, [_vp, _vp, _vp, _vp]),
        'magot_vcf_runs': (ctypes.c_int, [_vp, _vp, _vp, _vp]),
        'magot_vcf_resolve': (ctypes.c_int, [_vp, _vp, _vp, ctypes.c_uint64]),
        'magot_vcf_tables': (ctypes.c_int, [_vp] * 8),
        'magot_vcf_last_of': (ctypes.c_int, [_vp, _vp, ctypes.c_uint64, _u64p, _u64p, _u64p]),
        'magot_vcf_count': (ctypes.c_int, [_vp, _vp, _vp, _vp, _vp, ctypes.c_uint64, _vp, _vp,
                                           ctypes.POINTER(ctypes.c_uint32),
                                           ctypes.POINTER(ctypes.c_uint32)]),
        'magot_vcf_time': (ctypes.c_int, [_vp, _vp, ctypes.c_int, _vp, _u64p]),
        'magot_vcf_params': (None, [ctypes.POINTER(ctypes.c_uint32)] * 3 + [_u64p]),
        'magot_vcf_destroy': (None, [_vp]),
        'magot_vcf_render': (ctypes.c_int, [_vp, _vp, _vp, _vp, ctypes.c_uint64, ctypes.c_uint32,
                                            _vp, ctypes.c_uint32, ctypes.c_uint32,
                                            ctypes.POINTER(_vp), _u64p]),
        'magot_fastarec_parse': (ctypes.c_int, [_vp, _vp, ctypes.c_uint64, ctypes.c_uint32,
                                                ctypes.c_uint64, ctypes.POINTER(_vp),
                                                ctypes.POINTER(ctypes.c_uint32), _u64p]),
        'magot_fastarec_sizes': (ctypes.c_int, [_vp, _u64p, _u64p, _u64p, _u64p]),
        'magot_fastarec_upload_ms': (ctypes.c_double, [_vp]),
        'magot_fastarec_records': (ctypes.c_int, [_vp] * 11),
        'magot_fastarec_keys': (ctypes.c_int, [_vp] * 6),
        'magot_fastarec_exclude': (ctypes.c_int, [_vp, _vp, _vp, ctypes.c_uint64, _vp,
                                                  ctypes.c_uint64, ctypes.c_int, _vp]),
        'magot_fastarec_render': (ctypes.c_int, [_vp, _vp, _vp, ctypes.c_uint64, ctypes.c_uint32,
                                                 _u64p]),
        'magot_fastarec_render_fetch': (ctypes.c_int, [_vp, _vp, _vp, ctypes.c_uint64]),
        'magot_fastarec_time': (ctypes.c_int, [_vp, _vp, ctypes.c_int, _vp, _u64p, _u64p]),
        'magot_fastarec_params': (None, [ctypes.POINTER(ctypes.c_uint32)] * 3),
        'magot_fastarec_destroy': (None, [_vp]),
        'magot_rename_parse': (ctypes.c_int, [_vp, _vp, ctypes.c_uint64, _vp, _vp, _vp, _vp, _vp,
                                              ctypes.c_uint64, ctypes.c_uint32, ctypes.c_uint32,
                                              ctypes.c_uint64, ctypes.POINTER(_vp),
                                              ctypes.POINTER(ctypes.c_uint32)]),
        'magot_rename_sizes': (ctypes.c_int, [_vp, _u64p, _u64p, _u64p, _u64p]),
        'magot_rename_upload_ms': (ctypes.c_double, [_vp]),
        'magot_rename_hits': (ctypes.c_int, [_vp] * 4),
        'magot_rename_render': (ctypes.c_int, [_vp, _vp, _u64p]),
        'magot_rename_render_fetch': (ctypes.c_int, [_vp, _vp, _vp, ctypes.c_uint64]),
        'magot_rename_time': (ctypes.c_int, [_vp, _vp, ctypes.c_int, _vp, _u64p, _u64p]),
        'magot_rename_params': (None, [ctypes.POINTER(ctypes.c_uint32)] * 3),
        'magot_rename_destroy': (None, [_vp]),
        'magot_tabcut_parse': (ctypes.c_int, [_vp, _vp, ctypes.c_uint64, _vp, ctypes.c_uint32, _vp,
                                              ctypes.c_uint64, ctypes.c_uint32, ctypes.c_uint32,
                                              ctypes.c_uint32, ctypes.c_uint64,
                                              ctypes.POINTER(_vp),
                                              ctypes.POINTER(ctypes.c_uint32)]),
        'magot_tabcut_sizes': (ctypes.c_int, [_vp] + [_u64p] * 6),
        'magot_tabcut_upload_ms': (ctypes.c_double, [_vp]),
        'magot_tabcut_rows': (ctypes.c_int, [_vp] * 4),
        'magot_tabcut_render': (ctypes.c_int, [_vp, _vp, _u64p]),
        'magot_tabcut_render_fetch': (ctypes.c_int, [_vp, _vp, _vp, ctypes.c_uint64]),
        'magot_tabcut_time': (ctypes.c_int, [_vp, _vp, ctypes.c_int, _vp, _u64p, _u64p]),
        'magot_tabcut_params': (None, [ctypes.POINTER(ctypes.c_uint32)] * 3),
        'magot_tabcut_destroy': (None, [_vp]),
        'magot_gff_lower_write': (ctypes.c_int, [_vp, ctypes.c_uint32, ctypes.c_uint32, _u64p,
                                                 _u64p]),
        'magot_gffplan_write_views': (ctypes.c_int, [_vp, ctypes.POINTER(_vp), _u64p,
                                                     ctypes.POINTER(_vp), _u64p]),
        'magot_gffwrite_open': (ctypes.c_int, [_vp, _vp, ctypes.c_uint64, _vp, ctypes.c_uint64,
                                               _vp, ctypes.c_uint64, ctypes.c_uint64,
                                               ctypes.POINTER(_vp),
                                               ctypes.POINTER(ctypes.c_uint32), _u64p]),
        'magot_gffwrite_sizes': (ctypes.c_int, [_vp, _u64p, _u64p]),
        'magot_gffwrite_upload_ms': (ctypes.c_double, [_vp]),
        'magot_gffwrite_render': (ctypes.c_int, [_vp, _vp, _u64p]),
        'magot_gffwrite_render_fetch': (ctypes.c_int, [_vp, _vp, _vp, ctypes.c_uint64]),
        'magot_gffwrite_time': (ctypes.c_int, [_vp, _vp, ctypes.c_int, _vp, _u64p, _u64p]),
        'magot_gffwrite_params': (None, [ctypes.POINTER(ctypes.c_uint32)] * 3),
        'magot_gffwrite_destroy': (None, [_vp]),
    }
    for name, (res, args) in sig.items():
        fn = getattr(lib, name)
        fn.restype = res
        fn.argtypes = args
    return lib


def lib():
    """The loaded library (raises MagotError when it is not built)."""
    global _lib
    if _lib is None:
        with _lib_lock:
            if _lib is None:
                if not os.path.exists(LIB_PATH):
                    raise MagotError('libmagot.so not built at %s (run python -m magot_amd.build)'
                                     % LIB_PATH)
                _lib = _declare(ctypes.CDLL(LIB_PATH))
    return _lib


def check(rc, what):
    if rc != 0:
        msg = lib().magot_last_error().decode('utf-8', 'replace')
        raise MagotError('%s failed (status %d): %s' % (what, rc, msg))


def ptr(arr):
    """Address of a contiguous numpy array (or None for empty/None)."""
    if arr is None:
        return None
    return arr.ctypes.data_as(_vp)


class Context(object):
    """One device + one HIP stream (magot_ctx)."""

    def __init__(self, device=0):
        L = lib()
        n = L.magot_device_count()
        if n <= 0:
            raise MagotError('no HIP device visible: the MI355X extraction path needs a GPU')
        h = _vp()
        check(L.magot_ctx_create(int(device), ctypes.byref(h)), 'magot_ctx_create')
        self.handle = h
        self.device = int(device)

    def sync(self):
        check(lib().magot_ctx_sync(self.handle), 'magot_ctx_sync')

    def mark(self, which):
        """Record timing event `which` (0 = start, 1 = end) on the context
        stream (magot_ctx_mark)."""
        check(lib().magot_ctx_mark(self.handle, int(which)), 'magot_ctx_mark')

    def elapsed_ms(self):
        """GPU time between marks 0 and 1 (waits for mark 1)."""
        ms = ctypes.c_double()
        check(lib().magot_ctx_elapsed(self.handle, ctypes.byref(ms)), 'magot_ctx_elapsed')
        return ms.value

    def info(self):
        """{'n_cu', 'extract_blocks_per_cu'} of the device (magot_ctx_info)."""
        n_cu, blocks = ctypes.c_int(), ctypes.c_int()
        check(lib().magot_ctx_info(self.handle, ctypes.byref(n_cu), ctypes.byref(blocks)),
              'magot_ctx_info')
        return {'n_cu': n_cu.value, 'extract_blocks_per_cu': blocks.value}

    def close(self):
        if self.handle:
            lib().magot_ctx_destroy(self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


_default_ctx = None


def default_context():
    """Process-wide context on LOCAL_RANK's device (one process per GPU)."""
    global _default_ctx
    if _default_ctx is None:
        with _lib_lock:
            if _default_ctx is None:
                dev = int(os.environ.get('MAGOT_DEVICE', os.environ.get('LOCAL_RANK', '0')))
                _default_ctx = Context(dev)
    return _default_ctx
