"""GffRead.lower_cds (magot_gff_lower_cds, host code of libmagot.so: no device
needed) against the closed form of tests/cdspep_expect.py: the records'
intervals, names and transcript groups for every golden case in both orders,
and a decline on each diagnostic condition."""

import numpy as np
import pytest

import cdspep_expect as ce
from magot_amd import _lib, engine
from oracle import magot_oracle as mo


def lower(fasta, gff, order, **kw):
    seqs = mo.read_fasta(fasta)
    names = list(seqs)
    read = engine.GffRead.read(gff.encode('latin-1'))
    if read is None:  # read_gff returns None: no annotations, so no gene / transcript / CDS dict
        assert gff == ce.synthetic_gff(bad='no_annotations')
        return None, seqs, names
    flt = kw.get('gene_length_filter')
    plan = read.lower_cds(names, [len(seqs[n]) for n in names],
                          list(kw.get('gene_name_filters', ())),
                          None if flt is None else int(flt), kw.get('names_from', 'CDS'), order)
    return plan, seqs, names


@pytest.mark.parametrize('order', ['insertion', 'py2'])
@pytest.mark.parametrize('name', sorted(ce.TOOL_CASES))
def test_tables_and_names(name, order, golden_dir):
    fasta, gff, kw = ce.tool_inputs(name, golden_dir)
    if kw.get('names_from', 'CDS') not in _lib.CDS_NAMES:
        with pytest.raises(KeyError):  # the tool sends these to the object path
            lower(fasta, gff, order, **kw)
        return
    plan, seqs, names = lower(fasta, gff, order, **kw)
    if name in ('obiroi', 'no_annotations'):
        # mRNA children: annotations.transcript[...] is a KeyError; no annotations at
        # all: AttributeError
        assert plan is None
        return
    # the IndexError of a CDS without a candidate is no reason to decline: the
    # closed form is walked without it
    entries = []
    real = mo.get_orfs
    mo.get_orfs = lambda s, longest=False: ''
    try:
        entries, exc, _ = ce.walk(fasta, gff, order=order, **kw)
    finally:
        mo.get_orfs = real
    assert exc is None and plan is not None
    assert plan.n_records == len(entries) == len(plan.exons) == len(plan.txs)
    assert [b.decode('latin-1') for b in plan.name_list()] == [e[0] for e in entries]
    got = []
    for x in plan.exons:
        s = seqs[names[int(x['contig'])]]
        st = int(x['start_rc']) & ((1 << 63) - 1)
        piece = s[st:st + int(x['len'])]
        got.append(mo.reverse_complement(piece) if int(x['start_rc']) >> 63 else piece)
    assert got == [e[1] for e in entries]
    assert plan.txs['n_exons'].tolist() == [1] * len(entries)
    assert plan.txs['exon_begin'].tolist() == list(range(len(entries)))
    # groups: the records of one transcript
    tx_of = [e[2] for e in entries]
    grp = plan.group_off.astype(np.int64)
    assert grp[0] == 0 and grp[-1] == len(entries) and (np.diff(grp) >= 0).all()
    for g in range(len(grp) - 1):
        assert len(set(tx_of[grp[g]:grp[g + 1]])) <= 1
    assert sorted(set(tx_of)) == sorted({tx_of[a] for a in grp[:-1] if a < len(tx_of)})


@pytest.mark.parametrize('bad', sorted(ce.DIAGNOSTICS))
def test_declines_on_each_diagnostic_condition(bad):
    fasta = ce.synthetic_genome()
    kw = {'gene_length_filter': '10'} if bad == 'no_second_line' else {}
    assert lower(fasta, ce.synthetic_gff(), 'py2', **kw)[0] is not None
    assert lower(fasta, ce.synthetic_gff(bad=bad), 'py2', **kw)[0] is None
    # the condition sits in gene4: it declines although the filter drops that gene
    assert lower(fasta, ce.synthetic_gff(bad=bad), 'py2', gene_name_filters=['gene4'], **kw)[0] \
        is None or bad == 'no_second_line'


def test_a_replaced_cds_on_another_seqid_declines():
    gff = ce.synthetic_gff() + ce._line('ctgB', 'CDS', 2100, 2300, '-', 'ID=c4.other;Parent=t4.1')
    assert lower(ce.synthetic_genome(), gff, 'py2')[0] is None


def test_lowered_once():
    read = engine.GffRead.read(ce.synthetic_gff().encode('latin-1'))
    assert read.lower_cds(['ctgA', 'ctgB'], [3000, 2400]) is not None
    with pytest.raises(engine.MagotError):
        read.lower_cds(['ctgA', 'ctgB'], [3000, 2400])
