"""Time tab2fasta's and repeatmasker2augustushints' device passes, their host
loops and the whole tools on seeded synthetic tables made in memory.

    python scripts/tabcut_time.py --input transcriptome|wide|hints [--records 2000000]
                                  [--contigs 24] [--contig-mb 40] [--lines 5000000]
                                  [--iters 10] [--warmup 2] [--sample 20000] [--dir DIR]
                                  [--out profiles/tabcut_time.json]

One input per call, so that a caller can give every call a time limit of its
own and chain them; --out is read first and the input's entry replaced in it.

'transcriptome' (tab2fasta): what fasta2tab prints for the ``--records``
record transcriptome of scripts/fasta_time.py -- the same seeded headers and
sequences of 200 to 1200 bases, each record on one line.  'wide' (tab2fasta):
``--contigs`` lines with ``--contig-mb`` million bases in field 1 (the long-line
path: one lane per 4 KiB piece).  'hints' (repeatmasker2augustushints):
``--lines`` nine-column RepeatMasker GFF lines.

In this process, on the device: the whole engine.TabCut.parse call (wall) with
the upload's own event time, the render call (wall, the download included),
then ``warmup`` and ``iters`` runs of each pass with an event pair around it
(magot_tabcut_time) beside a device-to-device copy of the text; each pass is
also reported as a multiple of that copy.  On the host (wall): the tool's loop
(native='False') over the first ``--sample`` lines, scaled linearly to every
line -- an extrapolation, not a measurement; its bytes must be the head of the
device's.  Then the whole tool: the CLI call in a fresh child process on the
file written under --dir (wall, interpreter start and library load included),
under a time limit.  Needs a GPU; reads nothing outside the repository.  One
JSON document on stdout and in --out."""

import argparse
import contextlib
import io
import json
import os
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from magot_amd import engine, genome_tools  # noqa: E402

T0 = time.perf_counter()
CLI_LIMIT_S = 240


def note(msg):
    sys.stderr.write('[tabcut_time %6.1f s] %s\n' % (time.perf_counter() - T0, msg))
    sys.stderr.flush()


def transcriptome_tab(n_records, seed):
    """fasta2tab's output of fasta_time.transcriptome(n_records, ., seed): the
    same draws in the same order, each record as 'header TAB sequence LF'"""
    rng = np.random.default_rng(seed)
    pool = rng.choice(np.frombuffer(b'ACGT', np.uint8), 1 << 22).tobytes()
    lens = rng.integers(200, 1201, n_records).tolist()
    at = rng.integers(0, (1 << 22) - 1300, n_records).tolist()
    parts = []
    for r, (n, o) in enumerate(zip(lens, at)):
        parts.append(b'TRINITY_DN%d_c%d_g1_i%d len=%d path=[%d:0-%d]\t'
                     % (r // 3, r % 3, 1 + r % 2, n, o, n - 1))
        parts.append(pool[o:o + n])
        parts.append(b'\n')
    text = b''.join(parts)
    return text, {'lines': n_records, 'bytes': len(text), 'seed': seed}


def wide_tab(n_contigs, contig_mb, seed):
    rng = np.random.default_rng(seed)
    block = rng.choice(np.frombuffer(b'ACGTacgtN', np.uint8), contig_mb * 1000000).tobytes()
    parts = []
    for c in range(n_contigs):
        cut = (c * 7919) % 1000
        parts += [b'chr%d assembled\t' % (c + 1), block[cut:], block[:cut], b'\n']
    text = b''.join(parts)
    return text, {'lines': n_contigs, 'bytes': len(text), 'field_bytes': contig_mb * 1000000,
                  'seed': seed}


def hints_gff(n_lines, seed):
    rng = np.random.default_rng(seed)
    start = np.cumsum(rng.integers(50, 4000, n_lines))
    span = rng.integers(20, 3000, n_lines)
    score = rng.integers(200, 30000, n_lines)
    parts = [b'##gff-version 3\n']
    for k, (s, n, sc) in enumerate(zip(start.tolist(), span.tolist(), score.tolist())):
        parts.append(b'scaffold%d\tRepeatMasker\tsimilarity\t%d\t%d\t%d.%d\t%s\t.\t'
                     b'Target "Motif:rnd-%d_family-%d" %d %d\n'
                     % (k // 4000, s, s + n, sc // 10, sc % 10, b'+-'[k & 1:][:1], 1 + k % 6,
                        k % 997, 1 + k % 50, 1 + k % 50 + n))
    text = b''.join(parts)
    return text, {'lines': n_lines + 1, 'bytes': len(text), 'seed': seed}


def measure(label, tool, program, text, a, tmp):
    res = {}
    note('%s: parse, a warm-up then the timed call' % label)
    cut = engine.TabCut.parse(text, **program)
    assert isinstance(cut, engine.TabCut), cut
    cut.close()
    t = time.perf_counter()
    cut = engine.TabCut.parse(text, **program)
    cut.ctx.sync()
    res['parse_call_s'] = time.perf_counter() - t
    res['upload_ms'] = cut.upload_ms
    assert cut.short_line is None
    res.update(lines=cut.n_lines, tabs=cut.n_tabs, kept=cut.n_kept, pieces=cut.n_pieces,
               out_bytes=cut.out_bytes, text_bytes=len(text))
    t = time.perf_counter()
    out = cut.render()
    res['render_call_s'] = time.perf_counter() - t
    note('%s: timing the passes' % label)
    cut.time(a.warmup)
    ms = cut.time(a.iters)
    cut.close()
    res['passes_ms'] = {p: ms[p] for p in engine.TabCut.PASSES}
    copy = ms['copy']
    res['over_copy'] = {p: ms[p] / copy for p in engine.TabCut.PASSES[:-1]}
    res['copy_GBps'] = 2 * len(text) / copy / 1e6
    res['rows_ns_per_line'] = ms['rows'] * 1e6 / max(cut.n_lines, 1)

    note('%s: the host loop on a sample' % label)
    head = bytes(text[:64 << 20])
    cut_at, lines = -1, 0
    while lines < a.sample:
        nxt = head.find(b'\n', cut_at + 1)
        if nxt < 0:
            break
        cut_at, lines = nxt, lines + 1
    sample_path = os.path.join(tmp, 'sample.tab')
    with open(sample_path, 'wb') as fh:
        fh.write(head[:cut_at + 1])
    buf = io.TextIOWrapper(io.BytesIO(), encoding='latin-1', newline='\n')
    t = time.perf_counter()
    with contextlib.redirect_stdout(buf):
        tool(sample_path, native='False')
    loop_s = time.perf_counter() - t
    buf.flush()
    got = buf.buffer.getvalue()
    assert got == out[:len(got)].tobytes()  # the device printed the same for these lines
    res['host_loop'] = {'sample_lines': lines, 'sample_bytes': cut_at + 1, 'sample_s': loop_s,
                        'extrapolated_s': loop_s / max(cut_at + 1, 1) * len(text),
                        'note': 'extrapolated linearly in bytes from the sample; not a measurement'}
    n_out = len(out)
    del out

    note('%s: the CLI call in a process of its own' % label)
    path = os.path.join(tmp, label + '.tab')
    with open(path, 'wb') as fh:
        fh.write(text)
    env = dict(os.environ, MAGOT_CLI_TIMING='1',
               PYTHONPATH=ROOT + os.pathsep + os.environ.get('PYTHONPATH', ''))
    out_path = os.path.join(tmp, 'cut.out')
    with open(out_path, 'wb') as fh:
        t = time.perf_counter()
        child = subprocess.run([sys.executable, '-m', 'magot_amd.genome_tools', tool.__name__, path],
                               stdout=fh, stderr=subprocess.PIPE, env=env, timeout=CLI_LIMIT_S)
        wall = time.perf_counter() - t
    assert child.returncode == 0, child.stderr[-2000:]
    clock = json.loads(child.stderr.decode().strip().splitlines()[-1])
    assert os.path.getsize(out_path) == n_out
    res['cli_native'] = {'wall_s': wall, 'phases_s': clock['cli_phases_s'],
                         'total_s': clock['cli_total_s']}
    os.remove(path)
    os.remove(out_path)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--input', required=True, choices=('transcriptome', 'wide', 'hints'))
    ap.add_argument('--records', type=int, default=2000000)
    ap.add_argument('--contigs', type=int, default=24)
    ap.add_argument('--contig-mb', type=int, default=40)
    ap.add_argument('--lines', type=int, default=5000000)
    ap.add_argument('--iters', type=int, default=10)
    ap.add_argument('--warmup', type=int, default=2)
    ap.add_argument('--sample', type=int, default=20000)
    ap.add_argument('--seed', type=int, default=20261020)
    ap.add_argument('--dir')
    ap.add_argument('--out')
    a = ap.parse_args()
    res = {}
    if a.out and os.path.exists(a.out):
        with open(a.out) as fh:
            res = json.load(fh)
    res.update(iters=a.iters, warmup=a.warmup, params=engine.TabCut.params())
    with tempfile.TemporaryDirectory(dir=a.dir) as tmp:
        note('making the input')
        if a.input == 'transcriptome':
            text, shape = transcriptome_tab(a.records, a.seed)
            tool, program = genome_tools.tab2fasta, engine.TabCut.TAB2FASTA
        elif a.input == 'wide':
            text, shape = wide_tab(a.contigs, a.contig_mb, a.seed + 1)
            tool, program = genome_tools.tab2fasta, engine.TabCut.TAB2FASTA
        else:
            text, shape = hints_gff(a.lines, a.seed + 2)
            tool, program = genome_tools.repeatmasker2augustushints, engine.TabCut.HINTS
        res[a.input] = dict(measure(a.input, tool, program, text, a, tmp), text=shape,
                            tool=tool.__name__)
    text = json.dumps(res, indent=1, sort_keys=True)
    print(text)
    if a.out:
        with open(a.out, 'w') as fh:
            fh.write(text + '\n')
    return 0


if __name__ == '__main__':
    sys.exit(main())
