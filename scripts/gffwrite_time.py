"""Time convert_gff's native path and its parts on the C3 synthetic annotation.

    python scripts/gffwrite_time.py [--config C3] [--iters 10] [--warmup 2] [--sample 2000]
                                    [--dir DIR] [--out profiles/gffwrite_time.json]

The input is the workload's annotation in coordinate order (overlap_time's
write_annotation: a gene, an mRNA and its CDS lines per transcript, about 5 M
lines for C3), written under --dir (a temporary directory by default) and
removed at the end.

In this process: magot_gff_read without and with MAGOT_GFF_FOR_WRITE (wall
time, alternating, best and median of --reads runs each); then per output
format (gtf, gff3, exon_added_gff3): the lowering (wall time), the open call
(wall time: upload, size pass, scan) with the upload's own event time, the
render call (wall time, the launch and its completion) and the fetch of the text
to the host (wall time: into fresh pages, then twice into the same buffer),
then, after a warm-up, ``iters``
runs of each device pass with an event pair around it (magot_gffwrite_time)
beside a device-to-device copy of as many bytes as the render writes; the
render is reported as a multiple of that copy.  The object path
(genome.read_gff + write_gff) runs on the first --sample lines' worth of whole
genes and is reported per line only.  Then the whole tool: the CLI call in a
fresh child process.  Needs a GPU; reads nothing outside the repository.  One
JSON document on stdout and in --out."""

import argparse
import json
import os
import statistics
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'scripts'))

from magot_amd import engine, genome, synth  # noqa: E402
from overlap_time import write_annotation  # noqa: E402

T0 = time.perf_counter()
FORMATS = (('gtf', 'gtf'), ('gff3', 'simple gff3'), ('exon_added_gff3', 'exon added gff3'))


def note(msg):
    sys.stderr.write('[gffwrite_time %6.1f s] %s\n' % (time.perf_counter() - T0, msg))
    sys.stderr.flush()


def time_reads(data, runs):
    series = {'plain': [], 'for_write': []}
    for _ in range(runs):
        for name, flag in (('plain', False), ('for_write', True)):
            t = time.perf_counter()
            rd = engine.GffRead.read(data, for_write=flag)
            series[name].append(time.perf_counter() - t)
            assert rd is not None
            rd.close()
    return {k: {'runs_s': v, 'best_s': min(v), 'median_s': statistics.median(v)}
            for k, v in series.items()}


def measure(fmt, gff_format, data, read, path, a, tmp):
    res = {}
    t = time.perf_counter()
    plan = read.lower_write(gff_format, 'py2')
    res['lower_s'] = time.perf_counter() - t
    assert plan is not None
    res.update(rows=len(plan.rows), blob_bytes=len(plan.blob))
    t = time.perf_counter()
    w = engine.GffWriter.parse(data, plan.blob, plan.rows)
    res['open_call_s'] = time.perf_counter() - t
    assert isinstance(w, engine.GffWriter), w
    res['upload_ms'] = w.upload_ms
    res['out_bytes'] = w.out_bytes
    t = time.perf_counter()
    assert w.execute() == w.out_bytes
    res['render_call_s'] = time.perf_counter() - t
    out = np.empty(w.out_bytes, np.uint8)  # its pages are mapped by the first fetch
    fetches = []
    for _ in range(3):
        t = time.perf_counter()
        w.fetch(out)
        fetches.append(time.perf_counter() - t)
    res['fetch_s'] = {'first_s': fetches[0], 'again_s': fetches[1:]}
    res['fetch_GBps'] = w.out_bytes / min(fetches) / 1e9
    assert out[-1] == 10
    del out
    w.time(a.warmup)
    ms = w.time(a.iters)
    w.close()
    res['passes_ms'] = {p: ms[p] for p in engine.GffWriter.PASSES}
    res['render_over_copy'] = ms['render'] / ms['copy']
    res['render_GBps'] = w.out_bytes / ms['render'] / 1e6
    res['copy_GBps'] = 2 * w.out_bytes / ms['copy'] / 1e6
    note('%s: the CLI call in a process of its own' % fmt)
    env = dict(os.environ, MAGOT_CLI_TIMING='1',
               PYTHONPATH=ROOT + os.pathsep + os.environ.get('PYTHONPATH', ''))
    out_path = os.path.join(tmp, 'converted.' + fmt)
    with open(out_path, 'wb') as fh:
        t = time.perf_counter()
        child = subprocess.run([sys.executable, '-m', 'magot_amd.genome_tools', 'convert_gff',
                                path, 'gff3', fmt], stdout=fh, stderr=subprocess.PIPE, env=env)
        wall = time.perf_counter() - t
    assert child.returncode == 0, child.stderr[-2000:]
    assert os.path.getsize(out_path) == res['out_bytes']
    os.remove(out_path)
    res['cli_native'] = {'wall_s': wall}
    return res


def object_path(path, lines_wanted, fmts):
    """the object path on the first whole genes of the file, per line"""
    head = []
    with open(path) as fh:
        for ln in fh:
            if len(head) >= lines_wanted and '\tgene\t' in ln:
                break
            head.append(ln)
    text = ''.join(head)
    res = {'sample_lines': len(head)}
    t = time.perf_counter()
    aset = genome.read_gff(text)
    res['read_gff_us_per_line'] = (time.perf_counter() - t) * 1e6 / len(head)
    for fmt, gff_format in fmts:
        t = time.perf_counter()
        genome.write_gff(aset, gff_format, 'py2')
        res['write_gff_us_per_line_' + fmt] = (time.perf_counter() - t) * 1e6 / len(head)
    res['note'] = 'a sample, per line only; not scaled to the whole input'
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--config', default='C3')
    ap.add_argument('--tx', type=int, help='rescale the workload (rehearsals)')
    ap.add_argument('--genome-bases', type=int)
    ap.add_argument('--iters', type=int, default=10)
    ap.add_argument('--warmup', type=int, default=2)
    ap.add_argument('--reads', type=int, default=3)
    ap.add_argument('--sample', type=int, default=2000)
    ap.add_argument('--dir')
    ap.add_argument('--out')
    a = ap.parse_args()
    res = {'config': a.config, 'iters': a.iters, 'warmup': a.warmup,
           'params': engine.GffWriter.params()}
    with tempfile.TemporaryDirectory(dir=a.dir) as tmp:
        path = os.path.join(tmp, 'annotation.gff')
        note('building the workload tables')
        w = synth.make(a.config, order='sorted', genome=False, n_tx=a.tx,
                       genome_bases=a.genome_bases)
        note('writing the annotation')
        lines = write_annotation(path, w)
        res['text'] = {'lines': lines, 'bytes': os.path.getsize(path), 'transcripts': w.n_tx}
        data = genome.read_buffer(path)
        note('magot_gff_read with and without the flag')
        res['gff_read'] = time_reads(data, a.reads)
        read = engine.GffRead.read(data, for_write=True)
        for fmt, gff_format in FORMATS:
            note(fmt)
            res[fmt] = measure(fmt, gff_format, data, read, path, a, tmp)
        read.close()
        note('the object path on a sample')
        res['object_path'] = object_path(path, a.sample, FORMATS)
    text = json.dumps(res, indent=1, sort_keys=True)
    print(text)
    if a.out:
        with open(a.out, 'w') as fh:
            fh.write(text + '\n')
    return 0


if __name__ == '__main__':
    sys.exit(main())
