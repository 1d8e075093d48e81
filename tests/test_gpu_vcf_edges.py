"""vcf.hip's parse, sort and count passes at their own edges: the builders of
vcf_expect.py (what each holds is asserted in test_vcf_edges_expect.py) through
engine.VariantHets against the restated model, exactly, by test_gpu_vcf's
_assert_equals_table: line, pos, hash, bits, kept, first, the runs' and the
'##' lines' spans, the first variant's line, the counts and the foreign flag.

  (a) phases      every (start mod 16, length mod 16) of a data line
  (b) seams       tabs and fields on both sides of the 1,024-byte rounds of the
                  tab pass and of the 4,096-byte LDS stage, per start phase
  (c) chroms      CHROM against the data line before: the ballot up to 63
                  bytes, the loop from 64, shorter neighbours, an empty CHROM
  (d) table7/1024 the field table's chains, the wrap behind its last slot
  (e) kinds       the '#' line and the first data line on every lane of the
                  classify pass; texts without a last LF; a CR anywhere
  (f) sort/count  contig ids up to 2^32 - 1, up to 1,000 loci, piece edges
  (g) the loop    MAGOT_VCF_PARSE_GRID = 1, 2, 3, 64: a workgroup parses many
                  lines in a row, as it does above 2^20 data lines"""

import pytest

import test_gpu_vcf as base
import vcf_expect as ve
from magot_amd import engine, magot_variants

pytestmark = pytest.mark.gpu

GRIDS = ('1', '2', '3', '64')
HOOK = 'MAGOT_VCF_PARSE_GRID'


def _check(text, loci, order='py2', ids=None, timed=False):
    hets = base._native(text)
    try:
        want = base._assert_equals_table(hets, text, loci, order, ids)
        if timed:  # the replay of the passes goes through the same launch
            hets.time(1)
            base._assert_equals_table(hets, text, loci, order, ids)
        return want
    finally:
        hets.close()


def test_every_start_phase_and_length_class():
    text, loci = ve.phases()
    _check(text, loci, 'py2')
    _check(text, loci, 'insertion')


@pytest.mark.parametrize('skew', range(16))
def test_the_round_seams_and_the_stage_seam(skew):
    text, loci = ve.seams(skew)
    _check(text, loci, ve.ORDERS[skew % 2])


def test_chrom_against_the_line_before():
    text, loci = ve.chroms()
    _check(text, loci, 'py2')
    _check(text, loci, 'insertion')


def test_the_field_table_s_chains():
    _check(*ve.table7(), order='py2')
    _check(*ve.table7(), order='insertion')
    text, loci = ve.table1024()
    assert text.split('\n')[1].count('\t') == 8 + engine.VariantHets.params()[1]
    _check(text, loci, 'insertion')


@pytest.mark.parametrize('n_hdr', ve.HEADER_COUNTS)
def test_the_line_kinds_on_every_lane(n_hdr):
    text, loci = ve.kinds(n_hdr)
    hets = base._native(text)
    try:
        assert hets.n_header >= n_hdr and hets.header[0] == text.index('#CHROM')
        base._assert_equals_table(hets, text, loci, ve.ORDERS[n_hdr % 2])
    finally:
        hets.close()


def test_a_last_line_without_lf_at_every_length():
    for m in range(16):
        text, loci = ve.no_final_lf(m)
        _check(text, loci, ve.ORDERS[m % 2])


def test_a_cr_declines_wherever_it_stands():
    for label, with_cr, with_x in ve.cr_cases():
        assert engine.VariantHets.parse(with_cr.encode('latin-1')) == (None, 'carriage_return'), label
        _check(with_x, ve.CR_LOCI)


@pytest.mark.parametrize('ids', ve.ID_SETS, ids=['-'.join(map(str, i)) for i in ve.ID_SETS])
def test_contig_ids_of_every_width(ids):
    text, loci = ve.sort_text(), ve.sort_loci()
    named = dict(zip(ve.SORT_CHROMS, ids))
    _check(text, loci, 'py2', ids=named)
    _check(text, loci, 'insertion', ids=named)


@pytest.mark.parametrize('n', ve.LOCI_COUNTS)
def test_many_loci(n):
    named = {name: k for k, name in enumerate(ve.SORT_CHROMS)}
    _check(ve.sort_text(), ve.many_loci(n), 'py2', ids=named)


@pytest.mark.parametrize('k', range(5))
def test_keys_on_both_sides_of_a_piece_edge(k):
    split = engine.VariantHets.params()[0]
    text, loci = ve.pieces(ve.piece_counts(split)[k], split)
    _check(text, loci, ve.ORDERS[k % 2])


# ---------------------------------------------------------------------------
# the loop over the data lines
# ---------------------------------------------------------------------------

@pytest.mark.parametrize('grid', GRIDS)
def test_a_workgroup_parses_many_lines_in_a_row(grid, monkeypatch):
    monkeypatch.setenv(HOOK, grid)
    for skew in range(16):
        _check(*ve.seams(skew))
    _check(*ve.chroms())
    _check(*ve.table7())
    _check(*ve.table1024())
    _check(*ve.alternating())
    _check(*ve.world(257, 33), timed=True)
    _check(*ve.world(257, 130))


@pytest.mark.parametrize('value', ('', '0', '-1', '1048577', '2x', 'x', '99999999999999999999'))
def test_a_grid_outside_1_to_2_20_is_today_s(value, monkeypatch):
    monkeypatch.setenv(HOOK, value)
    _check(*ve.alternating())
    _check(*ve.world(257, 33))


def test_declines_name_the_lowest_line_under_any_grid(monkeypatch):
    cases = ve.decline_texts()
    for grid in (None, '1', '2'):
        if grid is None:
            monkeypatch.delenv(HOOK, raising=False)
        else:
            monkeypatch.setenv(HOOK, grid)
        for label, text, reason, line in cases:
            assert engine.VariantHets.parse(text.encode('latin-1')) == (None, reason), (grid, label)
            assert engine.VariantHets.last_declined_line == line, (grid, label)


# ---------------------------------------------------------------------------
# through the tool
# ---------------------------------------------------------------------------

@pytest.mark.parametrize('builder', ('phases', 'chroms', 'table7'))
def test_the_builders_through_the_tool(builder, tmp_path, capfd):
    text, loci = getattr(ve, builder)()
    path = str(tmp_path / 'calls.vcf')
    with open(path, 'wb') as fh:
        fh.write(text.encode('latin-1'))
    for order in ve.ORDERS:
        want = ve.expected(text, loci, 10000, order)
        got = base._run(lambda: magot_variants.heterozygosity_from_vcf(
            path, loci, 10000, order=order), capfd)
        assert got == want
        note = ve.native_note(text, loci, 10000, order)
        assert magot_variants.heterozygosity_from_vcf.last_path[1:] == \
            (('native', None) if note == 'native' else ('host', note))
