"""The edge builders of vcf_expect.py hold what they promise: every assertion
here is computed from the built text alone, without a device, and is what
keeps a test of test_gpu_vcf_edges.py from passing beside its point.

"Aligned offset" is the offset from the line's start rounded down to 16: the
quantity vcf.hip's parse pass compares with 1024 k (a round of its tab pass)
and 4096 (the end of its LDS stage)."""

import pytest

import vcf_expect as ve
from magot_amd import engine

NATIVE = ('native', 'foreign_name')
SPLIT, MOST_SAMPLES = engine.VariantHets.params()[:2]


def _aligned(start, i):
    return start % 16 + i


def _bits(text, loci):
    return ve.table(text, loci, 'insertion')['bits']


# ---------------------------------------------------------------------------
# (a)
# ---------------------------------------------------------------------------

def test_phases_hold_every_start_and_length_class():
    text, loci = ve.phases()
    assert ve.native_note(text, loci) in NATIVE
    data = ve.data_layout(text)
    assert all(len(f) == 11 and len(f[0]) == 1 and len(f[-1]) == 1 and f[8] == 'GT'
               for _, f, _ in data)
    length = [col[-1] + len(f[-1]) for _, f, col in data]
    assert {(start % 16, n % 16) for (start, _, _), n in zip(data, length)} == \
        {(p, q) for p in range(16) for q in range(16)}
    # a TAB of another line in the 16 aligned bytes of the line's first byte,
    # and in those of its last byte
    head, tail = set(), set()
    for (start, _, _), n in zip(data, length):
        last = start + n - 1
        if '\t' in text[start & ~15:start]:
            head.add(start % 16)
        if '\t' in text[last + 1:(last | 15) + 1]:
            tail.add(last % 16)
    assert head == set(range(3, 16)) and tail == set(range(13))
    t = ve.table(text, loci, 'py2')
    assert len(t['runs']) > 4 and 0 < sum(t['kept']) < len(data) and len(set(t['bits'])) == 2


# ---------------------------------------------------------------------------
# (b)
# ---------------------------------------------------------------------------

@pytest.mark.parametrize('skew', range(16))
def test_seams_hold_every_tab_place_and_every_split(skew):
    text, loci = ve.seams(skew)
    assert ve.native_note(text, loci) in NATIVE
    data = ve.data_layout(text)
    bits = _bits(text, loci)
    assert all(start % 16 == skew and len(f) == 12 for start, f, _ in data)
    tabs = {(k, _aligned(start, col[k] - 1)) for start, f, col in data for k in ve.SEAM_TAB_FIELDS}
    assert tabs >= {(k, at) for k in ve.SEAM_TAB_FIELDS for at in ve.SEAM_TABS}
    # bytes of the field before aligned offset 4096, per kind of straddler
    seen = {kind: set() for kind in ve.STRADDLERS}
    for (start, f, col), row_bits in zip(data, bits):
        for k in range(8, 12):
            before = ve.STAGE - _aligned(start, col[k])
            if not 0 <= before <= len(f[k]):
                continue
            if k == 8 and f[8] == ve.STRADDLERS['format']:
                seen['format'].add(before)
                assert row_bits  # its GT is found behind the seam
            if k > 8 and f.index(f[k]) == k and f[8] == 'DP:GT':
                for kind in ('het', 'hom', 'ten'):
                    if f[k] == ve.STRADDLERS[kind]:
                        seen[kind].add(before)
                        assert (row_bits >> (k - 9) & 1) == (kind == 'het')
            if k == 11 and 9 <= f.index(f[k]) < k and f[k] == ve.STRADDLERS['equal']:
                earlier = f.index(f[k])
                assert _aligned(start, col[earlier] + len(f[k])) <= ve.STAGE  # wholly staged
                seen['equal'].add(before)
                assert row_bits >> (earlier - 9) & 1 and not row_bits >> 2 & 1
    for kind, v in ve.STRADDLERS.items():
        assert seen[kind] == set(range(len(v) + 1)), kind
    # '7:10/1': a split puts the first and the last byte of its GT on two sides
    assert ve.STRADDLERS['ten'].split(':')[1][0] == ve.STRADDLERS['ten'][-1]
    rounds = [{_aligned(start, c - 1) // ve.ROUND for c in col[1:]} for start, _, col in data]
    spread = [f for (_, f, _), r in zip(data, rounds) if len(r) == 4]
    assert any(len(f[2]) >= 1100 and len(f[7]) >= 1100 and f[3:7] == [''] * 4 for f in spread)


# ---------------------------------------------------------------------------
# (c)
# ---------------------------------------------------------------------------

def _is_head(prev, f):
    return prev is None or prev[0] != f[0]


def test_chroms_hold_every_length_and_every_neighbour():
    text, loci = ve.chroms()
    assert ve.native_note(text, loci) == 'native'
    data = ve.data_layout(text)
    assert all(len(f) == 10 for _, f, _ in data)
    assert min(col[-1] + len(f[-1]) for _, f, col in data) == 21  # an empty CHROM's line
    fields = [f for _, f, _ in data]
    chrom = [f[0] for f in fields]
    size = [col[-1] + len(f[-1]) for _, f, col in data]
    for n in ve.CHROM_LENGTHS:
        d = next(d for d, c in enumerate(chrom) if len(c) == n and chrom[d + 1] == c)
        x = chrom[d]
        assert chrom[d + 1] == x
        assert chrom[d + 2][:-1] == x[:-1] and chrom[d + 2][-1] != x[-1] and len(chrom[d + 2]) == n
        assert chrom[d + 3][1:] == x[1:] and chrom[d + 3][0] != x[0] and len(chrom[d + 3]) == n
        assert chrom[d + 4] == x + 'z' and chrom[d + 5] == x and chrom[d + 6] == 'c'
        assert chrom[d + 7] == x and (size[d + 6] < n) == (n > 22) and size[d + 6] == 22
        # keys come again in a later run of X
        assert fields[d + 5][1] == fields[d][1] and fields[d + 7][1] == fields[d + 1][1]
    assert {n for n in ve.CHROM_LENGTHS if n >= 64} and {n for n in ve.CHROM_LENGTHS if n in (62, 63)}
    differ = set()
    for a, b in zip(chrom, chrom[1:]):
        if len(a) == len(b) == 70 and a != b:
            at = [j for j in range(70) if a[j] != b[j]]
            if len(at) == 1:
                differ.add(at[0])
    assert differ == set(ve.CHROM_PAIRS) == {62, 63, 64}
    empty = [d for d, c in enumerate(chrom) if c == '']
    assert len(empty) == 2 and empty[1] == empty[0] + 1
    # a '##' line and a blank line inside a run
    lines = [ln for _, ln in ve.split_lines(text)]
    inside = [k for k in range(1, len(lines) - 2) if lines[k][:2] == '##' and lines[k + 1] == '']
    assert inside and lines[inside[0] - 1].split('\t')[0] == lines[inside[0] + 2].split('\t')[0]
    # CHROMs that end around the stage seam: the separator and POS straddle it
    for skew in ve.CHROM_SEAM_SKEWS:
        ends = {len(f[0]) for start, f, _ in data if start % 16 == skew and len(f[0]) > 4000}
        assert ends >= set(ve.CHROM_SEAM)
        across = [f for start, f, _ in data if start % 16 == skew and
                  _aligned(start, len(f[0]) + 1) < ve.STAGE < _aligned(start, len(f[0]) + 1 + len(f[1]))]
        assert across
    assert any(a == b and len(a) > ve.STAGE for a, b in zip(chrom, chrom[1:]))
    t = ve.table(text, loci, 'py2')
    heads = sum(_is_head(p, f) for p, f in zip([None] + fields[:-1], fields))
    assert len(t['runs']) == heads and 0 < sum(t['kept']) < len(data)
    assert sum(t['first']) == sum(t['kept']) and t['first'] != t['kept']


# ---------------------------------------------------------------------------
# (d)
# ---------------------------------------------------------------------------

def test_the_restated_hash_is_fnv1a():
    assert ve.fnv1a('') == 2166136261 and ve.fnv1a('a') == 0xe40c292c  # the published vectors
    assert ve.fnv1a('foobar') == 0xbf9cf968
    assert sum(ve.fnv1a('0/1:%d' % d) & 31 == 31 for d in range(2000)) == 66
    assert (ve.table_slots(7), ve.table_slots(MOST_SAMPLES)) == (32, 4096) and MOST_SAMPLES == 1024
    import numpy as np
    assert ve.fnv1a_numbered('1/1:', 1000).tolist() == [ve.fnv1a('1/1:%07d' % d) for d in range(1000)]
    assert np.uint64(0xffffffff) * np.uint64(16777619) < np.uint64(2 ** 63)


def test_table7_holds_its_chains():
    text, loci = ve.table7()
    assert ve.native_note(text, loci) in NATIVE
    rows = [f for _, f, _ in ve.data_layout(text)]
    assert all(len(f) == 16 for f in rows)
    home = lambda c: ve.fnv1a(c) & 31  # noqa: E731
    bits = _bits(text, loci)
    wrapped = 0
    for f, row_bits in zip(rows, bits):
        last = [c for c in dict.fromkeys(f[9:]) if home(c) == 31]
        # under any order of claims at most one of them sits in slot 31: of two
        # repeated ones, one is found behind the wrap
        again = {c for s, c in enumerate(f[9:]) if f.index(c) != 9 + s and c in last}
        if len(last) >= 5 and len(again) >= 2:
            wrapped += 1
            for s, c in enumerate(f[9:]):
                assert (row_bits >> s & 1) == (f.index(c) == 9 + s and c[0] != c[2])
    assert wrapped == 2 and bits[0] and not bits[4]
    fixed = {home(x) for x in rows[1][:9]}
    assert len(set(rows[1][9:])) == 7 and all(home(c) in fixed for c in rows[1][9:])
    assert len(set(rows[2][9:])) == 1 and bits[2] == 1
    assert rows[3][9] == rows[3][15] and len(set(rows[3][9:])) == 6 and bits[3] & 0x41 == 1


def test_table1024_holds_its_chain_and_its_repeats():
    text, loci = ve.table1024()
    assert ve.native_note(text, loci) in NATIVE
    rows = [f for _, f, _ in ve.data_layout(text)]
    assert [len(f) for f in rows] == [9 + MOST_SAMPLES] * 3
    calls = rows[1][9:]
    last = {c for c in calls if ve.fnv1a(c) & 4095 == 4095}
    assert len(last) >= 256 and {c[:3] for c in last} == {'0/1', '1/1'}
    first = {}
    for s, c in enumerate(calls):
        first.setdefault(c, s)
    again = [s for s, c in enumerate(calls) if first[c] != s]
    assert len(again) >= 200
    assert all(sum(lo <= s < lo + 128 for s in again) >= 10 for lo in range(0, 1024, 128))
    assert sum(calls[s] in last for s in again) >= 20  # repeats along the chain too
    assert all(sum(first[c] // 128 == k for c in last) >= 10 for k in range(8))
    assert len(set(rows[0][9:])) == len(set(rows[2][9:])) == 1024


# ---------------------------------------------------------------------------
# (e)
# ---------------------------------------------------------------------------

@pytest.mark.parametrize('n_hdr', ve.HEADER_COUNTS)
def test_kinds_put_the_lines_on_their_lanes(n_hdr):
    text, loci = ve.kinds(n_hdr)
    assert ve.native_note(text, loci) in NATIVE
    lines = [ln for _, ln in ve.split_lines(text)]
    assert all(ln[:2] == '##' for ln in lines[:n_hdr]) and lines[n_hdr][:2] == '#C'
    assert lines[n_hdr + 1][:1] in 'cd'
    data = [k for k, ln in enumerate(lines) if ln and ln[0] != '#']
    assert len(data) == ve.KINDS_DATA
    # a line that is neither behind the data lines d with ...
    gap = {d for d, (a, b) in enumerate(zip(data, data[1:])) if b - a > 1}
    assert gap >= set(range(8)) | {62, 63, 125, 127, 188, 191}
    between = [lines[k] for a, b in zip(data, data[1:]) for k in range(a + 1, b)]
    assert '' in between and any(ln[:2] == '##' for ln in between)
    assert sum(ln[:2] == '##' for ln in lines) > n_hdr


def test_the_header_counts_reach_every_lane_of_the_classify_pass():
    # the '#' line is line H, the first data line H + 1: lane 0, lane 63, the
    # first lane of a second wave and of a second workgroup of 256
    at = set(ve.HEADER_COUNTS) | {h + 1 for h in ve.HEADER_COUNTS}
    assert at >= {0, 1, 63, 64, 255, 256, 257} and max(at) > 512
    assert {h % 64 for h in ve.HEADER_COUNTS} >= {0, 63} <= {(h + 1) % 64 for h in ve.HEADER_COUNTS}
    assert {h % 256 for h in ve.HEADER_COUNTS} >= {0, 255} <= {(h + 1) % 256 for h in ve.HEADER_COUNTS}


def test_texts_without_a_last_lf_and_texts_with_a_cr():
    for m in range(16):
        text, loci = ve.no_final_lf(m)
        assert len(text) % 16 == m and text[-1] != '\n' and ve.native_note(text, loci) == 'native'
    cases = ve.cr_cases()
    assert len(cases) == 32
    middle = {a.index('\r') % 16 for label, a, _ in cases if label.startswith('at_')}
    ends = {len(a) % 16 for label, a, _ in cases if label.startswith('last_')}
    assert middle == ends == set(range(16))
    for label, a, b in cases:
        assert a.count('\r') == 1 and len(a) == len(b) and '\r' not in b
        at = a.index('\r')
        assert a[:at] == b[:at] and a[at + 1:] == b[at + 1:] and b[at] == 'x'
        assert (at == len(a) - 1) == label.startswith('last_')
        assert ve.native_note(a, ve.CR_LOCI) == 'carriage_return'
        assert ve.native_note(b, ve.CR_LOCI) == 'native'


# ---------------------------------------------------------------------------
# (f)
# ---------------------------------------------------------------------------

def test_the_sort_text_and_its_loci():
    text, loci = ve.sort_text(), ve.sort_loci()
    assert ve.native_note(text, loci) in NATIVE
    rows = [f for _, f, _ in ve.data_layout(text)]
    assert len(rows) == 257 and {f[0] for f in rows} == set(ve.SORT_CHROMS)
    for c in ve.SORT_CHROMS:
        pos = [int(f[1]) for f in rows if f[0] == c]
        assert pos.count(0) > 1 and pos.count(77) > 1 and pos.count(ve.INT_MAX) > 1
        assert '%s,9' % c in loci and '%s,77,77' % c in loci and '%s,5,4' % c in loci
        assert '%s,%d,%d' % (c, ve.INT_MAX, 2 ** 32 - 1) in loci
    # the same POS on two CHROMs: ids that join two names join keys
    assert len({(f[0], f[1]) for f in rows}) > len({f[1] for f in rows})
    plain = ve.table(text, loci, 'py2')
    for ids in ve.ID_SETS:
        t = ve.table(text, loci, 'py2', ids=dict(zip(ve.SORT_CHROMS, ids)))
        assert (len(set(ids)) == 3) == (t['kept'] == plain['kept'] and t['counts'] == plain['counts'])
        assert t['pos'] == plain['pos'] and t['hash'] == plain['hash'] and t['bits'] == plain['bits']
    tops = [max(ids) for ids in ve.ID_SETS]
    assert [t.bit_length() for t in tops] == [0, 1, 2, 3, 9, 17, 32, 32]
    assert {1, 3, 4, 255, 256, 65535, 65536, 2 ** 31 - 1, 2 ** 31, 2 ** 32 - 2, 2 ** 32 - 1} <= \
        {i for ids in ve.ID_SETS for i in ids}
    # ids=None is the model as it was: every name its own contig
    assert ve.table(text, loci, 'py2', ids={c: c for c in ve.SORT_CHROMS})['counts'] == plain['counts']


@pytest.mark.parametrize('n', ve.LOCI_COUNTS)
def test_many_loci_hold_long_empty_runs(n):
    text, loci = ve.sort_text(), ve.many_loci(n)
    assert len(loci) == n
    counts = ve.table(text, loci, 'py2')['counts']
    held = [any(row) for row in counts]
    assert held[0]
    if n == 1:
        return
    assert sum(held) >= n // 60 and not any(held[-3:]) and len(set(loci)) < n
    runs = ''.join('x' if h else '.' for h in held).split('x')
    assert max(map(len, runs)) >= 50 and sum(len(r) >= 50 for r in runs) >= min(n // 60, 3)
    assert any(loci[k] == loci[k + 1] and held[k] for k in range(n - 1))


def _edges(text, loci):
    """per locus the piece edges [(kept of the row before, kept of the row
    behind, whether both have one key)] of its rows of the sorted lines"""
    t = ve.table(text, loci, 'py2')
    order = sorted(range(len(t['pos'])), key=lambda d: (t['pos'][d], d))
    out = []
    for locus in loci:
        f = locus.split(',')
        lo = int(f[1]) if len(f) > 2 else 0
        rows = [d for d in order if t['pos'][d] >= lo]
        out.append([(t['kept'][rows[e - 1]], t['kept'][rows[e]], t['pos'][rows[e - 1]] == t['pos'][rows[e]])
                    for e in range(SPLIT, len(rows), SPLIT)])
    return out, t


def test_pieces_split_keys_at_their_edges():
    twins = [0, 0]
    for n in ve.piece_counts(SPLIT):
        text, loci = ve.pieces(n, SPLIT)
        assert ve.native_note(text, loci) == 'native'
        edges, t = _edges(text, loci)
        assert len(t['pos']) == n and 0 < sum(t['kept']) < n and len(t['runs']) == 1
        assert [len(e) for e in edges] == [(n - 1) // SPLIT, (n - 2) // SPLIT]
        assert sorted(t['pos'])[1] == int(loci[1].split(',')[1]) > min(t['pos'])
        for k in (0, 1):
            twins[k] += sum(e == (0, 1, True) for e in edges[k])
    # an unkept row ends a piece and its kept twin starts the next: for the
    # whole contig's pieces and for those of the locus from the second row on
    assert twins[0] >= 3 and twins[1] >= 1


# ---------------------------------------------------------------------------
# (g)
# ---------------------------------------------------------------------------

def test_alternating_lines_and_declines():
    text, loci = ve.alternating()
    assert ve.native_note(text, loci) in NATIVE
    data = ve.data_layout(text)
    size = [col[-1] + len(f[-1]) for _, f, col in data]
    equal = [len(set(f[9:])) == 1 for _, f, _ in data]
    assert len(data) == 20 and {len(set(f[9:])) for _, f, _ in data} == {1, 5}
    assert all((a > 8192) != (b > 8192) and min(a, b) <= 40 for a, b in zip(size, size[1:]))
    assert {(a > 8192, b) for a, b in zip(size, equal)} == {(x, y) for x in (0, 1) for y in (0, 1)}
    cases = ve.decline_texts()
    assert len(cases) == 3 * len(ve.DECLINES) + 2
    assert {c[2] for c in cases} == {'field_count', 'chrom_form', 'pos_form', 'pos_range', 'no_gt',
                                     'empty_gt', 'equals_fixed'}
    few = [len(ve.DECLINES[k][1]) for k in ('few_tabs', 'many_tabs')]
    assert few == [10, 12]
    for label, text, reason, line in cases:
        assert ve.native_note(text, ['c,100']) == reason, label
        assert ve.first_decline(text) == (reason, line)
        data = ve.data_layout(text)
        assert len(data) == 40
        bad = [d for d, (_, f, _) in enumerate(data) if ve._line_reason(f, 2)]
        assert bad in ([0], [20], [39], [10, 30])
        if len(bad) == 2:
            assert ve._line_reason(data[30][1], 2) not in (None, reason)
