"""Every device slice of a tool's handle is rounded up to 256 bytes, so a count
that lost its ``+ 1`` or took the wrong length shows only where
``n * sizeof(T)`` is an exact multiple of 256.  For the eight tools below:
inputs whose line count, and inputs whose record, key or data-line count, is
exactly 32, 64 and 256 (8-, 4- and 1-byte elements fill their slice to the last
byte there), through the tool on the device and through its host loop, which
must print the same bytes."""

import pytest

import depth_expect as de
import fqstats_expect as fe
import overlap_expect as oe
import psl_expect as pe
import vcf_expect as vx
from magot_amd import genome_tools

pytestmark = pytest.mark.gpu

EDGES = (32, 64, 256)


def b(text):
    return text.encode('latin-1')


def lines_in(data):
    return data.count(b'\n') + (1 if data and not data.endswith(b'\n') else 0)


# -- one builder per tool: (files, call) with `n_lines` lines and `n_rec` records

PSL_HEAD = b'psLayout version 3\n\nmatch\tmis- \n     \tmatch\n---------\n'  # five lines


def psl(n_lines, n_rec):
    head = PSL_HEAD if n_lines > n_rec else b''
    assert n_lines == n_rec + lines_in(head)
    keys = max(1, n_rec * 3 // 4)  # a quarter of the queries have two lines
    body = b''.join(pe.psl_line(100 + (7 * i) % 50, i % 9, 'query%d' % (i % keys))
                    for i in range(n_rec))
    text = head + body
    assert sum(1 for ln in text.split(b'\n')[:-1] if ln[:1].isdigit()) == n_rec
    return [text], lambda p, **kw: genome_tools.besthits_from_psl(p[0], **kw)


def _fasta(n_lines, n_rec):
    """n_rec records of distinct names over n_lines lines: every record has a
    sequence line, the first ones a second"""
    extra = n_lines - 2 * n_rec
    assert 0 <= extra <= n_rec
    out = []
    for r in range(n_rec):
        out.append(b'>rec%d some words\n' % r + b'ACGTTGCA' * (1 + r % 5) + b'\n')
        if r < extra:
            out.append(b'GGCC' * (1 + r % 3) + b'\n')
    text = b''.join(out)
    assert text.count(b'>') == n_rec
    return text


def exclude(n_lines, n_rec):
    listed = b''.join(b'rec%d some words\n' % r for r in range(0, n_rec, 3)) + b'absent\n'
    return [_fasta(n_lines, n_rec), listed], \
        lambda p, **kw: genome_tools.exclude_from_fasta(p[0], p[1], **kw)


def tab(n_lines, n_rec):
    return [_fasta(n_lines, n_rec)], lambda p, **kw: genome_tools.fasta2tab(p[0], **kw)


def rename(n_lines, n_rec):
    """n_rec table rows of distinct names, a text of n_lines lines whose fields
    end in ';': every other field is a name"""
    table = b''.join(b'n%03dx\tV%03d\tnote\n' % (k, k) for k in range(n_rec))
    text = b''.join(b'n%03dx;other%d;xn%03dx;tail\n' % (i % n_rec, i, (i * 7) % n_rec)
                    for i in range(n_lines))
    assert lines_in(table) == n_rec
    return [text, table], lambda p, **kw: genome_tools.replace_names(p[0], p[1], ';', **kw)


def vcf(n_lines, n_rec):
    calls = ('0/1:5', '0/0:6', '1/1:7', '0|1:3', '1/2:4')
    rows = [vx.row('c1', 10 + 90 * i, *[calls[(i + s) % 5] for s in range(3)])
            for i in range(n_rec)]
    text = b(vx.vcf(rows))  # three header lines
    assert n_lines == n_rec + 3
    assert sum(1 for ln in text.split(b'\n') if ln and ln[:1] != b'#') == n_rec
    return [text], lambda p, **kw: genome_tools.heterozygosity_from_vcf(p[0], **kw)


def depth(n_lines, n_rec):
    """a depth table of n_lines lines over two contigs, and n_rec CDS rows"""
    first = n_lines // 2
    contigs = [('ctgA', de.formula_depths(first, 7, 41)),
               ('ctgB', de.formula_depths(n_lines - first, 5, 37, 3))]
    tx = []
    for t in range(n_rec // 2):  # two CDS each, inside contig A
        a = 1 + (3 * t) % max(1, first - 8)
        tx.append(('tx%d' % t, 'ctgA', '+-'[t % 2], [(a, a + 2), (a + 4, a + 6)]))
    gff = b(de.gff_text(tx))
    assert gff.count(b'\tCDS\t') == n_rec
    return [de.table_text(contigs), gff], \
        lambda p, **kw: genome_tools.depth_from_gff(p[0], p[1], features="['CDS','upstream']",
                                                    stream_length='5', **kw)


def fastq(n_lines, n_rec):
    assert n_lines == 4 * n_rec
    text = b''.join(fe.record(b'r%d' % i, 1 + (11 * i) % 23) for i in range(n_rec))
    return [text], lambda p, **kw: genome_tools.fqstats(p[0], **kw)


def purge(n_lines, n_rec):
    """n_rec intervals to purge with, n_lines lines to purge"""
    first = b''.join(oe.gff_line('s%d' % (i % 3), 100 * i + 10, 100 * i + 60) for i in range(n_rec))
    second = b''.join(oe.gff_line('s%d' % (i % 4), 50 * i + 1, 50 * i + 20) for i in range(n_lines))
    assert lines_in(first) == n_rec
    return [first, second], lambda p, **kw: genome_tools.purge_overlaps(p[0], p[1], **kw)


# tool -> (builder, (lines, records) with `lines` at the edge n, the same with `records` there)
TOOLS = {
    'besthits_from_psl': (psl, lambda n: (n, n - 5), lambda n: (n, n)),
    'exclude_from_fasta': (exclude, lambda n: (n, n // 2), lambda n: (2 * n + n // 4, n)),
    'fasta2tab': (tab, lambda n: (n, n // 2 - 3), lambda n: (2 * n, n)),
    'replace_names': (rename, lambda n: (n, n - 1), lambda n: (n, n)),
    'heterozygosity_from_vcf': (vcf, lambda n: (n, n - 3), lambda n: (n + 3, n)),
    'depth_from_gff': (depth, lambda n: (n, 6), lambda n: (n, n)),
    'fqstats': (fastq, lambda n: (n, n // 4), lambda n: (4 * n, n)),
    'purge_overlaps': (purge, lambda n: (n, n - 1), lambda n: (n, n)),
}
# where the tool reads its line count from (the file that is indexed by lines)
LINE_FILE = {'purge_overlaps': 1}
CASES = [(tool, which, n) for tool in TOOLS for which in ('lines', 'records') for n in EDGES]


def _run(call, paths, capfdbinary, native):
    exc = None
    try:
        call(paths, native=native)
    except Exception as e:  # noqa: BLE001
        exc = type(e).__name__
    return capfdbinary.readouterr().out, exc


@pytest.mark.parametrize('tool,which,n', CASES, ids=['%s-%s%d' % c for c in CASES])
def test_the_device_prints_the_host_loops_bytes_at_the_slice_edges(tool, which, n, tmp_path,
                                                                   capfdbinary):
    build, at_lines, at_records = TOOLS[tool]
    n_lines, n_rec = (at_lines if which == 'lines' else at_records)(n)
    files, call = build(n_lines, n_rec)
    assert lines_in(files[LINE_FILE.get(tool, 0)]) == n_lines
    assert (n_lines if which == 'lines' else n_rec) == n  # the builders assert their records
    paths = []
    for k, data in enumerate(files):
        paths.append(str(tmp_path / ('in%d' % k)))
        with open(paths[-1], 'wb') as fh:
            fh.write(data)
    capfdbinary.readouterr()
    want = _run(call, paths, capfdbinary, 'False')
    assert getattr(genome_tools, tool).last_path[1] == 'host'
    got = _run(call, paths, capfdbinary, 'True')
    assert getattr(genome_tools, tool).last_path[1] == 'native', getattr(genome_tools, tool).last_path
    assert want[1] is None and want[0]
    assert got == want
