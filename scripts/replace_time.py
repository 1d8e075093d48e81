"""Time replace_names' device passes and the whole tool on the C3 synthetic
annotation renamed from a table of its gene IDs.

    python scripts/replace_time.py [--config C3] [--iters 20] [--warmup 3] [--sample 8]
                                   [--dir DIR] [--out profiles/replace_time.json]

The text is the workload's annotation in coordinate order (overlap_time's
write_annotation: a gene, an mRNA and its CDS lines per transcript, about 5 M
lines for C3).  Two tables with one row per transcript and ``name_end=';'``:
``hits`` renames every ``gene<N>`` (it occurs once as ``ID=gene<N>;``), ``none``
lists as many names of the same shape that do not occur.  Both are written under
--dir (a temporary directory by default) and removed at the end.

In this process, per table: the table read and the decision on the host (wall
time), the parse call (wall time: upload, table build, field ends, match and
layout) with the upload's own event time, the render call (wall time, the
download included), then, after a warm-up, ``iters`` runs of each device pass
with an event pair around it (magot_rename_time) beside a device-to-device copy
of the text; the matching pass is reported as a multiple of that copy.  The
reference's loop restated (genome_tools._replace_host) runs over the first
--sample lines that hold a hit and is scaled linearly to every line: that
figure is an extrapolation, not a measurement; its output must equal the
device's for those lines.  Then the whole tool: the CLI call in a fresh child
process.  Needs a GPU; reads nothing outside the repository.  One JSON document
on stdout and in --out."""

import argparse
import json
import os
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'scripts'))

from magot_amd import engine, genome, genome_tools, synth  # noqa: E402
from overlap_time import write_annotation  # noqa: E402

T0 = time.perf_counter()
D = b';'


def note(msg):
    sys.stderr.write('[replace_time %6.1f s] %s\n' % (time.perf_counter() - T0, msg))
    sys.stderr.flush()


def measure(name, text_path, table_path, lines, a, tmp):
    res = {}
    t = time.perf_counter()
    with open(table_path, 'rb') as fh:
        rows = genome_tools._replace_table(fh.read())
    res['table_read_s'] = time.perf_counter() - t
    t = time.perf_counter()
    why, table = genome_tools._replace_decline(rows, D, 'py2')
    res['decision_s'] = time.perf_counter() - t
    assert why is None, why
    names, values, rank = table
    data = genome.read_buffer(text_path)
    note('%s: the parse call' % name)
    t = time.perf_counter()
    rep = engine.NameReplacer.parse(data, names, values, D, rank)
    res['parse_call_s'] = time.perf_counter() - t
    assert isinstance(rep, engine.NameReplacer), rep
    res['upload_ms'] = rep.upload_ms
    res.update(lines=rep.n_lines, fields=rep.n_fields, hits=rep.n_hits, out_bytes=rep.out_bytes,
               text_bytes=len(data), names=len(names))
    t = time.perf_counter()
    out = rep.render()
    res['render_call_s'] = time.perf_counter() - t
    note('%s: timing the passes' % name)
    rep.time(a.warmup)
    ms = rep.time(a.iters)
    rep.close()
    res['passes_ms'] = {p: ms[p] for p in engine.NameReplacer.PASSES}
    copy = ms['copy']
    res['over_copy'] = {p: ms[p] / copy for p in ('field_ends', 'match', 'layout', 'render')}
    res['match_ns_per_field'] = ms['match'] * 1e6 / max(rep.n_fields, 1)
    res['copy_GBps'] = 2 * len(data) / copy / 1e6

    note('%s: the host loop on a sample' % name)
    head = bytes(data[:1 << 20])
    sample = [ln for ln in head.split(b'\n')[:-1] if b'ID=gene' in ln][:a.sample]
    sample_text = b'\n'.join(sample) + b'\n'
    keys, vals = genome_tools._replace_dict(rows, D, 'py2')
    t = time.perf_counter()
    got = b''.join(genome_tools._replace_host(sample_text, [k + D for k in keys],
                                              [v + D for v in vals]))
    loop_s = time.perf_counter() - t
    if name == 'hits':  # the device printed the same for these lines
        whole = out.tobytes()
        assert all(ln + b'\n' in whole for ln in got.split(b'\n')[:-1] if ln)
        assert got != sample_text
    else:
        assert got == sample_text
    res['host_loop'] = {'sample_lines': len(sample), 'sample_s': loop_s,
                        'extrapolated_s': loop_s / max(len(sample), 1) * lines,
                        'note': 'extrapolated linearly from the sample; not a measurement'}
    del data, out

    note('%s: the CLI call in a process of its own' % name)
    env = dict(os.environ, MAGOT_CLI_TIMING='1',
               PYTHONPATH=ROOT + os.pathsep + os.environ.get('PYTHONPATH', ''))
    out_path = os.path.join(tmp, 'renamed.gff')
    with open(out_path, 'wb') as fh:
        t = time.perf_counter()
        child = subprocess.run([sys.executable, '-m', 'magot_amd.genome_tools', 'replace_names',
                                text_path, table_path, 'name_end=;'],
                               stdout=fh, stderr=subprocess.PIPE, env=env)
        wall = time.perf_counter() - t
    assert child.returncode == 0, child.stderr[-2000:]
    clock = json.loads(child.stderr.decode().strip().splitlines()[-1])
    assert os.path.getsize(out_path) == res['out_bytes']
    res['cli_native'] = {'wall_s': wall, 'phases_s': clock['cli_phases_s'],
                         'total_s': clock['cli_total_s']}
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--config', default='C3')
    ap.add_argument('--tx', type=int, help='rescale the workload (rehearsals)')
    ap.add_argument('--genome-bases', type=int)
    ap.add_argument('--iters', type=int, default=20)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--sample', type=int, default=8)
    ap.add_argument('--dir')
    ap.add_argument('--out')
    a = ap.parse_args()
    res = {'config': a.config, 'iters': a.iters, 'warmup': a.warmup, 'name_end': ';',
           'params': engine.NameReplacer.params()}
    with tempfile.TemporaryDirectory(dir=a.dir) as tmp:
        text_path = os.path.join(tmp, 'annotation.gff')
        note('building the workload tables')
        w = synth.make(a.config, order='sorted', genome=False, n_tx=a.tx,
                       genome_bases=a.genome_bases)
        note('writing the annotation')
        lines = write_annotation(text_path, w)
        res['text'] = {'lines': lines, 'bytes': os.path.getsize(text_path), 'transcripts': w.n_tx}
        for name, row in (('hits', 'gene%d\tMAGOT%07d\tx\n'), ('none', 'locus%d\tMAGOT%07d\tx\n')):
            table_path = os.path.join(tmp, name + '.tsv')
            with open(table_path, 'w') as fh:
                fh.write(''.join(row % (t, t) for t in range(w.n_tx)))
            res[name] = measure(name, text_path, table_path, lines, a, tmp)
    text = json.dumps(res, indent=1, sort_keys=True)
    print(text)
    if a.out:
        with open(a.out, 'w') as fh:
            fh.write(text + '\n')
    return 0


if __name__ == '__main__':
    sys.exit(main())
