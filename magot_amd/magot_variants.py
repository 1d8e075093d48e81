"""magot_variants.py of the reference: ``read_vcf`` and
``calculate_heterozygosity`` (magot_variants.py:16-139), and
``heterozygosity_from_vcf``, which gives the same prints and the same string
from the VCF's text on the device.

The reference builds one object per genotype and then walks every variant
against every locus of its contig.  On the device (engine.VariantHets) the text
is parsed once, a wave per data line, into a sorted table of (contig, POS) keys
and one het bit per sample column; every locus is then a range of that table.

Python 2 shows in four places, all restated here: ``list(set(loci))`` and
``list(variant_set)`` follow CPython 2.7's slot order (py2order; a 2.7 set
probes and grows as a dict does), ``seqlen / window`` floors, ``str`` of a
float keeps twelve significant digits, and a printed list shows ``repr`` of byte
strings.  ``order='insertion'`` gives first-seen order instead of slot order.
"""

import copy
import re
import sys

import numpy as np

from . import engine
from . import genome
from . import py2order
from .genome import Genotype, Variant, VariantSet

_INT = re.compile(r'^-?[0-9]{1,18}$')
_PY_SPACE = ' \t\n\r\x0b\x0c'


def _py2_int(text):
    """int() of a str as Python 2 reads it: surrounding whitespace, one
    optional sign, decimal digits (no '_' separators)."""
    s = text.strip(_PY_SPACE)
    digits = s[1:] if s[:1] in ('+', '-') else s
    if not digits or not digits.isdigit() or not digits.isascii():
        raise ValueError('invalid literal for int() with base 10: %r' % text)
    return int(s)


def _py2_float_str(value):
    text = '%.12g' % value
    return text if ('.' in text or 'e' in text or 'n' in text) else text + '.0'


def _py2_repr(s):
    """repr of a Python 2 byte string (here a str of latin-1 characters)."""
    quote = '"' if ("'" in s and '"' not in s) else "'"
    out = [quote]
    for ch in s:
        o = ord(ch)
        if ch == quote or ch == '\\':
            out.append('\\' + ch)
        elif ch == '\t':
            out.append('\\t')
        elif ch == '\n':
            out.append('\\n')
        elif ch == '\r':
            out.append('\\r')
        elif o < 0x20 or o >= 0x7f:
            out.append('\\x%02x' % o)
        else:
            out.append(ch)
    out.append(quote)
    return ''.join(out)


def _py2_list_repr(names):
    return '[' + ', '.join(_py2_repr(n) for n in names) + ']'


def _check_order(order):
    if order not in ('py2', 'insertion'):
        raise ValueError("order must be 'py2' or 'insertion'")


def _distinct(keys, order):
    """list(set(keys)) (``order='py2'``) or the distinct keys as first seen."""
    if order == 'py2':
        return py2order.dict_order(keys)
    return list(dict.fromkeys(keys))


def _dict_keys(d, order, copies=0):
    keys = list(d)
    return py2order.order_after_copies(keys, copies) if order == 'py2' else keys


def _emit(*items):
    for it in items:
        sys.stdout.write(str(it) + '\n')


def _header_loci(header_text, window):
    """magot_variants.py:25-34: the windows of every ``##contig=<ID=`` line."""
    locus_list = []
    for vcf_header_line in header_text.split('\n'):
        if "##contig=<ID=" in vcf_header_line:
            seqid = vcf_header_line.split(',')[0][13:]
            seqlen = _py2_int(vcf_header_line.split(',')[1][7:-1])
            seqchunk_number = seqlen // window
            for seqchunk in range(seqchunk_number):
                locus_list.append(seqid + ',' + str(1 + window * seqchunk) + ',' +
                                  str(window * (seqchunk + 1)))
            locus_list.append(seqid + ',' + str(1 + window * seqchunk_number) + ',' + str(seqlen))
    return locus_list


def calculate_heterozygosity(variant_set, locus_list=None, window=10000, order='py2'):
    """magot_variants.py:16-88.  Loci are ``seqid,seq_length`` for a whole
    contig or ``seqid,start,stop`` (inclusive); without a list they are the
    windows of the header's contig lines.  Prints ``built locus list``, the
    number of loci and the sample names; returns one row per locus of positive
    length: the locus and per sample 100 * (het variants inside) / length."""
    _check_order(order)
    outlist = []
    if locus_list is None:
        if variant_set.vcf_headers is not None:
            locus_list = _header_loci(variant_set.vcf_headers[0], window)
        else:
            _emit("function run with out locus_list, but variant_set has no vcf_header. One day "
                  "I'll add a             function to get loci from a GenomeSequence; if you "
                  "really want this, pester me about it on github 'Issues'")
            return None
    locus_list = _distinct(locus_list, order)
    _emit("built locus list", len(locus_list))
    variant_codes = _dict_keys(variant_set, order)
    locus_het_count_dic = {}
    loci_dic = {}
    for locus in locus_list:
        locus_het_count_dic[locus] = {}
        for genotype in variant_set[variant_codes[0]].genotypes:
            locus_het_count_dic[locus][genotype] = 0
        seqid = locus.split(',')[0]
        if seqid in loci_dic:
            loci_dic[seqid].append(locus)
        else:
            loci_dic[seqid] = [locus]
    for variant_code in variant_codes:
        variant_code_split = variant_code.split('<:>')
        seqid = variant_code_split[0]
        position = _py2_int(variant_code_split[1])
        for locus in loci_dic[seqid]:
            locus_split = locus.split(',')
            if len(locus_split) > 2:
                if _py2_int(locus_split[1]) <= position <= _py2_int(locus_split[2]):
                    inside = True
                else:
                    inside = False
            else:
                inside = True
            if inside:
                genotypes = variant_set[variant_code].genotypes
                for genotype in genotypes:
                    genotypeGT = genotypes[genotype].GT
                    if genotypeGT[0] != genotypeGT[-1]:
                        locus_het_count_dic[locus][genotype] = \
                            locus_het_count_dic[locus][genotype] + 1
    standard_genotype_list = None
    for locus in locus_list:
        if standard_genotype_list is None:
            # the genotypes dict was deep-copied once and re-inserted once
            standard_genotype_list = _dict_keys(locus_het_count_dic[locus], order, copies=2)
            _emit(_py2_list_repr(standard_genotype_list))
        locus_split = locus.split(',')
        if len(locus_split) > 2:
            seqlen = _py2_int(locus_split[2]) - _py2_int(locus_split[1]) + 1
        else:
            seqlen = _py2_int(locus_split[1])
        if seqlen >= 1:
            hetrate_list = []
            for genotype in standard_genotype_list:
                hetrate_list.append(_py2_float_str(100.0 * locus_het_count_dic[locus][genotype]
                                                   / seqlen))
            outlist.append(locus + "," + ",".join(hetrate_list))
    return '\n'.join(outlist)


def read_vcf(vcf, variant_set_to_modify=None):
    """magot_variants.py:91-139: a VCF (a path, a file object or the text)
    into a VariantSet keyed ``CHROM<:>POS``."""
    # read_to_string (magot_smallfuncs.py:46-56) drops every CR of the text
    vcf_list = genome._read_source(vcf).replace('\r', '').split('\n')
    vcf_headerlines = []
    if variant_set_to_modify is None:
        variant_set = VariantSet()
    else:
        variant_set = variant_set_to_modify
    if variant_set.vcf_headers is None:
        variant_set.vcf_headers = []
    vcf_header_index = len(variant_set.vcf_headers)
    for line in vcf_list:
        if line == "":
            pass
        elif line[:2] == "##":
            vcf_headerlines.append(line)
        elif line[0] == "#":
            field_names = line[1:].split('\t')
            if len(field_names) > 8:
                sample_names = field_names[9:]
        else:
            fields = line.split('\t')
            seqid = fields[0]
            position = fields[1]
            ref_allele = fields[3]
            alt_alleles = fields[4].split(',')
            variant_ID = seqid + "<:>" + position
            variant = Variant(ref_allele, alt_alleles, variant_set=variant_set)
            variant.ID = fields[2]
            variant.quality = fields[5]
            variant.filter_status = fields[6]
            variant.info = fields[7]
            variant.vcf_header_index = vcf_header_index
            variant_set[variant_ID] = variant
            if len(fields) > 8:
                genotypes = {}
                sample_features = fields[8].split(':')
                for sample in fields[9:]:
                    # a name before the '#' line: UnboundLocalError, as there
                    sample_name = sample_names[fields.index(sample) - 9]
                    genotypes[sample_name] = Genotype()
                    this_sample_features = sample.split(':')
                    for feature in sample_features:
                        try:
                            setattr(genotypes[sample_name], feature,
                                    this_sample_features[sample_features.index(feature)])
                        except IndexError:
                            pass
                variant.genotypes = copy.deepcopy(genotypes)
    variant_set.vcf_headers.append('\n'.join(vcf_headerlines))
    if variant_set_to_modify is None:
        return variant_set


# ---------------------------------------------------------------------------
# the device path
# ---------------------------------------------------------------------------

_U32_MAX = 0xffffffff


def _locus_rows(locus_list):
    """Per locus (seqid, lo, hi, seqlen) with [lo, hi] the positions it
    holds clamped to 0 .. 2^32 - 1 (lo > hi: none); None when a locus is outside
    what the device path takes: two or more comma fields, the numbers
    ``-?digits`` of at most 18 digits."""
    rows = []
    for locus in locus_list:
        f = locus.split(',')
        if len(f) < 2 or not _INT.match(f[1]) or (len(f) > 2 and not _INT.match(f[2])):
            return None
        if len(f) > 2:
            start, stop = int(f[1]), int(f[2])
            seqlen = stop - start + 1
            lo, hi = max(start, 0), min(stop, _U32_MAX)
            if lo > hi:
                lo, hi = 1, 0
        else:
            seqlen = int(f[1])
            lo, hi = 0, _U32_MAX
        rows.append((f[0], lo, hi, seqlen))
    return rows


def _line_names(line, sample_names):
    """The names of a data line's genotypes dict in insertion order, each with
    the column it was first credited from (read_vcf's ``fields.index``)."""
    fields = line.split('\t')
    names = {}
    for sample in fields[9:]:
        col = fields.index(sample) - 9
        names.setdefault(sample_names[col], col)
    return names


def _native(vcf, locus_list, window, order):
    """(prints, result or exception, None) from the device, or (None, None,
    reason) when only the host path is exact."""
    data = genome.read_buffer(vcf)
    hets = engine.VariantHets.parse(data)
    if isinstance(hets, tuple):
        return None, None, hets[1]
    try:
        text = memoryview(data)

        def span(off, length):
            return bytes(text[int(off):int(off) + int(length)]).decode('latin-1')

        sample_names = span(*hets.header)[1:].split('\t')[9:]
        if len(set(sample_names)) != len(sample_names):
            return None, None, 'duplicate_names'
        if locus_list is None:
            if not isinstance(window, int) or isinstance(window, bool):
                return None, None, 'window_form'
            off, length = hets.header_lines()
            header = '\n'.join(span(o, n) for o, n in zip(off.tolist(), length.tolist()))
            try:
                locus_list = _header_loci(header, window)
            except (ValueError, IndexError, ZeroDivisionError, MemoryError, OverflowError):
                return None, None, 'header_form'
        else:
            locus_list = list(locus_list)
            if not all(isinstance(x, str) for x in locus_list):
                return None, None, 'locus_form'
        locus_list = _distinct(locus_list, order)
        rows = _locus_rows(locus_list)
        if rows is None:
            return None, None, 'locus_form'
        prints = ['built locus list', str(len(locus_list))]
        # contigs: the run heads' CHROM spans against the loci's seqids
        seq_ids = {}
        for seqid, _, _, _ in rows:
            seq_ids.setdefault(seqid, len(seq_ids))
        r_off, r_len = hets.runs()
        contig_of_run = np.zeros(len(r_off), np.uint32)
        for k, (o, n) in enumerate(zip(r_off.tolist(), r_len.tolist())):
            name = span(o, n)
            if name not in seq_ids:
                return prints, KeyError(name), None
            contig_of_run[k] = seq_ids[name]
        hets.resolve(contig_of_run)
        _, off, length = hets.first_variant_line(order)
        names = _line_names(span(off, length), sample_names)
        allowed = np.zeros(hets.words, np.uint32)
        for col in names.values():
            allowed[col >> 5] |= np.uint32(1 << (col & 31))
        counts, foreign = hets.count(np.array([seq_ids[r[0]] for r in rows], np.uint32),
                                     np.array([r[1] for r in rows], np.uint32),
                                     np.array([r[2] for r in rows], np.uint32), allowed)
        if counts is None:
            return None, None, foreign
        if foreign:
            return None, None, 'foreign_name'
        std = py2order.order_after_copies(list(names), 2) if order == 'py2' else list(names)
        prints.append(_py2_list_repr(std))
        cols = np.array([names[n] for n in std], np.int64)
        result = engine.render_hets(locus_list, np.array([r[3] for r in rows], np.int64),
                                    counts, cols)
        return prints, result, None
    finally:
        hets.close()


def heterozygosity_from_vcf(vcf, locus_list=None, window=10000, order='py2', native='True'):
    """``calculate_heterozygosity(read_vcf(vcf), locus_list, window)``: the same
    three prints, the same string, the same exception types.

    On the device (engine.VariantHets) when ``vcf`` names a regular file inside
    the native grammar: exactly one ``#`` line that is not ``##``, before the
    first data line and with at least one sample, all names distinct; every
    data line of 9 + S fields, no CR anywhere (read_vcf drops every CR before it
    splits the text, so a CRLF file is the host path's), CHROM without ``<:>``, POS 1 to 10 digits with no
    leading zero and at most 2^31 - 1, a FORMAT that holds ``GT``, every sample
    column with a non-empty GT subfield and different from fields 0 to 8; at
    least one data line; loci of two or more fields with plain integers; no het
    of a sample that the first variant lacks inside a locus.  Otherwise, and
    with ``native=False``, the two functions above answer.  A CHROM without a
    locus raises KeyError from the device path, after the first two prints.
    Nothing is printed before the path is known.
    ``heterozygosity_from_vcf.last_path`` names the path the last call took."""
    import os
    _check_order(order)
    if native != 'True':
        why = "native != 'True'"
    elif not (isinstance(vcf, str) and os.path.isfile(vcf)):
        why = 'not a regular file'
    else:
        prints, result, why = _native(vcf, locus_list, window, order)
        if why is None:
            heterozygosity_from_vcf.last_path = ('heterozygosity_from_vcf', 'native', None)
            _emit(*prints)
            if isinstance(result, Exception):
                raise result
            return result
    heterozygosity_from_vcf.last_path = ('heterozygosity_from_vcf', 'host', why)
    return calculate_heterozygosity(read_vcf(vcf), locus_list, window, order=order)


heterozygosity_from_vcf.last_path = None
