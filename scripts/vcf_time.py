"""Time heterozygosity_from_vcf's device passes, its host steps and the whole
tool on a seeded synthetic cohort VCF made in memory.

    python scripts/vcf_time.py [--lines 1250000] [--samples 100] [--iters 10] [--warmup 2]
                               [--sample 400] [--window 10000] [--dir DIR]
                               [--out profiles/vcf_time.json]

The text: a header of ten ``##contig`` lines of 100 Mb each (1 Gb in all) and
the '#' line, then ``--lines`` data lines sorted by contig and position,
positions drawn evenly from 10^7 .. 10^8 - 1 (eight digits: every line has one
width), FORMAT ``GT:DP``, ``--samples`` columns ``<GT>:<100 + column>`` with GT
drawn from 0/0, 0/1, 1/1, 1/2 -- the depth keeps a line's columns distinct, so
every line names every sample.  At the defaults the text is about 1.05 GB,
beyond the 256 MiB cache; with ``--window 10000`` there are 100,010 loci.

In this process, on the device: ``warmup`` then ``iters`` runs of each pass with
an event pair around it (magot_vcf_time; device ms) and of a device-to-device
copy of the text; the parse pass's bytes per second against the copy's, both
over the text's own bytes; the upload inside one parse; the whole
engine.VariantHets.parse call three times (wall time).  On the host (wall time,
three runs each): the loci from the header, their Python 2 set order, the first
variant from the hashes, the renderer.  The host path (read_vcf +
calculate_heterozygosity) on the first ``--sample`` data lines with the whole
header, its time scaled to the whole text by lines (the loop is variants x loci
of the contig) and marked as an extrapolation.  Then the whole tool: the CLI call
in a fresh child process on the text written under --dir (wall time, interpreter
start and library load included).  Needs a GPU; reads nothing outside the
repository.  One JSON document on stdout and in --out."""

import argparse
import contextlib
import json
import os
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from magot_amd import engine, magot_variants as mv  # noqa: E402

T0 = time.perf_counter()
CONTIGS, CONTIG_LEN = 10, 100000000


def note(msg):
    sys.stderr.write('[vcf_time %6.1f s] %s\n' % (time.perf_counter() - T0, msg))
    sys.stderr.flush()


def synth_vcf(n_lines, n_samples, seed):
    """(header bytes, body as an n_lines x width uint8 array)"""
    rng = np.random.default_rng(seed)
    head = ['##fileformat=VCFv4.2']
    head += ['##contig=<ID=chr%02d,length=%d>' % (c + 1, CONTIG_LEN) for c in range(CONTIGS)]
    head.append('\t'.join(['#CHROM', 'POS', 'ID', 'REF', 'ALT', 'QUAL', 'FILTER', 'INFO', 'FORMAT'] +
                          ['smp%03d' % s for s in range(n_samples)]))
    header = ('\n'.join(head) + '\n').encode('latin-1')
    fixed = b'chr00\t00000000\t.\tA\tC\t50\tPASS\tDP=9\tGT:DP'
    row = fixed + b''.join(b'\t0/0:%03d' % (100 + s) for s in range(n_samples)) + b'\n'
    body = np.tile(np.frombuffer(row, np.uint8), (n_lines, 1))
    contig = np.sort(rng.integers(0, CONTIGS, n_lines))
    pos = rng.integers(10 ** 7, 10 ** 8, n_lines)
    order = np.lexsort((pos, contig))
    contig, pos = contig[order], pos[order]
    body[:, 3] = 48 + (contig + 1) // 10
    body[:, 4] = 48 + (contig + 1) % 10
    for k in range(8):
        body[:, 6 + k] = 48 + pos // 10 ** (7 - k) % 10
    cols = body[:, len(fixed):len(fixed) + 8 * n_samples].reshape(n_lines, n_samples, 8)
    gt = rng.integers(0, 4, (n_lines, n_samples), dtype=np.uint8)
    cols[:, :, 1] = np.array([48, 48, 49, 49], np.uint8)[gt]
    cols[:, :, 3] = np.array([48, 49, 49, 50], np.uint8)[gt]
    hets = int(((gt == 1) | (gt == 3)).sum())
    return header, body, hets


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--lines', type=int, default=1250000)
    ap.add_argument('--samples', type=int, default=100)
    ap.add_argument('--iters', type=int, default=10)
    ap.add_argument('--warmup', type=int, default=2)
    ap.add_argument('--sample', type=int, default=400)
    ap.add_argument('--window', type=int, default=10000)
    ap.add_argument('--seed', type=int, default=20261020)
    ap.add_argument('--dir')
    ap.add_argument('--out')
    a = ap.parse_args()
    res = {'iters': a.iters, 'warmup': a.warmup, 'window': a.window}
    note('making the text')
    header, body, het_calls = synth_vcf(a.lines, a.samples, a.seed)
    text = np.concatenate([np.frombuffer(header, np.uint8), body.reshape(-1)])
    width = body.shape[1]
    del body
    n = len(text)
    res['text'] = {'bytes': n, 'data_lines': a.lines, 'samples': a.samples, 'line_bytes': width,
                   'contigs': CONTIGS, 'contig_length': CONTIG_LEN, 'het_calls': het_calls,
                   'seed': a.seed, 'order': 'sorted by contig and position'}

    note('parse: warm-up, then three calls')
    hets = engine.VariantHets.parse(text)
    assert isinstance(hets, engine.VariantHets), hets
    hets.close()
    walls, uploads = [], []
    for k in range(3):
        t = time.perf_counter()
        hets = engine.VariantHets.parse(text)
        walls.append(time.perf_counter() - t)
        uploads.append(hets.upload_ms)
        if k < 2:
            hets.close()
    assert (hets.n_data, hets.n_samples, hets.n_runs) == (a.lines, a.samples, CONTIGS)
    res['parse_call_wall_s'] = walls
    res['upload_device_ms'] = uploads
    res['upload_GBps'] = [n / ms / 1e6 for ms in uploads]

    note('the host steps')
    off, length = hets.header_lines()
    view = memoryview(text)
    head_text = '\n'.join(bytes(view[int(o):int(o) + int(m)]).decode('latin-1')
                          for o, m in zip(off.tolist(), length.tolist()))
    loci_s, order_s, first_s, render_s = [], [], [], []
    for _ in range(3):
        t = time.perf_counter()
        loci = mv._header_loci(head_text, a.window)
        loci_s.append(time.perf_counter() - t)
        t = time.perf_counter()
        loci = mv._distinct(loci, 'py2')
        rows = mv._locus_rows(loci)
        order_s.append(time.perf_counter() - t)
    seq_ids = {}
    for r in rows:
        seq_ids.setdefault(r[0], len(seq_ids))
    r_off, r_len = hets.runs()
    runs = [bytes(view[int(o):int(o) + int(m)]).decode('latin-1')
            for o, m in zip(r_off.tolist(), r_len.tolist())]
    hets.resolve([seq_ids[name] for name in runs])
    for _ in range(3):
        t = time.perf_counter()
        hets.first_variant_line('py2')
        first_s.append(time.perf_counter() - t)
    allowed = np.full(hets.words, 0xffffffff, np.uint32)
    t = time.perf_counter()
    counts, foreign = hets.count(np.array([seq_ids[r[0]] for r in rows], np.uint32),
                                 np.array([r[1] for r in rows], np.uint32),
                                 np.array([r[2] for r in rows], np.uint32), allowed)
    res['count_call_wall_s'] = time.perf_counter() - t
    assert not foreign and int(counts.sum(dtype=np.int64)) <= het_calls
    res['loci'] = len(loci)
    res['het_calls_counted'] = int(counts.sum(dtype=np.int64))  # less the replaced duplicates
    seqlen = np.array([r[3] for r in rows], np.int64)
    for _ in range(3):
        t = time.perf_counter()
        out = engine.render_hets(loci, seqlen, counts, np.arange(a.samples))
        render_s.append(time.perf_counter() - t)
    res['host'] = {'header_loci_wall_s': loci_s, 'py2_set_order_and_rows_wall_s': order_s,
                   'first_variant_wall_s': first_s, 'render_wall_s': render_s,
                   'runs_each': 3}
    res['output_bytes'] = len(out)

    note('timing the passes')
    hets.time(a.warmup)
    ms = hets.time(a.iters)
    res['passes_device_ms'] = {k: ms[k] for k in engine.VariantHets.PASSES}
    res['passes_device_ms']['total_without_copy'] = sum(ms[k] for k in engine.VariantHets.PASSES
                                                        if k != 'copy')
    # both over the text's own bytes: the copy also writes them once
    res['parse_GBps'] = n / ms['parse'] / 1e6
    res['copy_GBps_of_text'] = n / ms['copy'] / 1e6
    res['parse_over_copy_time'] = ms['parse'] / ms['copy']
    res['parse_ns_per_line'] = ms['parse'] * 1e6 / a.lines
    hets.close()

    with tempfile.TemporaryDirectory(dir=a.dir) as tmp:
        note('the host path on a sample')
        cut = len(header) + a.sample * width
        sample_path = os.path.join(tmp, 'sample.vcf')
        with open(sample_path, 'wb') as fh:
            fh.write(view[:cut])
        with open(os.devnull, 'w') as null, contextlib.redirect_stdout(null):
            t = time.perf_counter()
            mv.heterozygosity_from_vcf(sample_path, None, a.window, native='False')
            loop_s = time.perf_counter() - t
        assert mv.heterozygosity_from_vcf.last_path[1] == 'host'
        res['host_path'] = {'sample_lines': a.sample, 'sample_wall_s': loop_s, 'runs': 1,
                            'extrapolated_s': loop_s / a.sample * a.lines,
                            'note': 'the whole text at the sample\'s time per data line (every '
                                    'line is walked against the 10,001 loci of its contig): an '
                                    'extrapolation, not a measurement'}

        note('the CLI call in a process of its own')
        path = os.path.join(tmp, 'calls.vcf')
        with open(path, 'wb') as fh:
            fh.write(view)
        env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get('PYTHONPATH', ''))
        out_path = os.path.join(tmp, 'hets.csv')
        with open(out_path, 'wb') as fh:
            t = time.perf_counter()
            child = subprocess.run([sys.executable, '-m', 'magot_amd.genome_tools',
                                    'heterozygosity_from_vcf', path, 'window=%d' % a.window],
                                   stdout=fh, stderr=subprocess.PIPE, env=env)
            wall = time.perf_counter() - t
        assert child.returncode == 0, child.stderr[-2000:]
        with open(out_path, 'rb') as fh:
            got = fh.read()
        # the three prints, then the rows (their columns in the names' Python 2 order)
        assert got.startswith(b'built locus list\n%d\n[' % len(loci))
        assert len(got) == len(b'built locus list\n%d\n' % len(loci)) + 10 * a.samples + 1 + \
            len(out) + 1
        res['cli_native'] = {'wall_s': wall, 'runs': 1}
    doc = json.dumps(res, indent=1, sort_keys=True)
    print(doc)
    if a.out:
        with open(a.out, 'w') as fh:
            fh.write(doc + '\n')
    return 0


if __name__ == '__main__':
    sys.exit(main())
