"""Time composition_by_site's counting pass, its host steps and the whole tool on
two seeded synthetic alignments near one device plane.

    python scripts/site_time.py [--tall 100000x30000] [--wide 16x200000000] [--only tall|wide]
                                [--iters 20] [--warmup 3] [--sample-cells 3000000] [--dir DIR]
                                [--out profiles/site_time.json]

The alignments, ROWSxSITES each: 'tall', many short rows (the pass splits the
rows into strips and adds their counts with atomics), and 'wide', few long
rows (one strip, the counts are stored).  Every row is a window of one seeded
pool of bases (uniform ACGT, 3 % of them soft-masked in runs of 50, 2 % gaps in
runs of 10, 0.5 % N) that starts at a seeded offset, written as a one-line
FASTA record.

Per alignment, in this process: the native read, upload and pack
(engine.FastaGenome.load, wall time to a device synchronise); ``warmup`` then
``iters`` runs of the pass between an event pair (engine.SiteCounts.time;
device ms), as a rate of nibble bytes (0.5 byte per cell) and of all bytes the
pass must move (the nibbles and 16 bytes of counts per site), each against
8 TB/s; the counts checked against numpy on seeded columns; the fetch of the
counts and the renderer (wall time).  Then the tool's host loop
(native='False') on the first rows and sites that make ``--sample-cells``
cells, its rate per cell scaled to the whole alignment and marked as an
extrapolation; and the whole tool: the CLI call in a fresh child process on
the text written under --dir (wall time, interpreter start and library load
included), its output compared with the text rendered in this process.  Needs a GPU; reads nothing outside the repository.  One JSON
document on stdout and in --out."""

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
sys.path.insert(0, os.path.join(ROOT, 'tests'))

import site_expect as se  # noqa: E402
from magot_amd import engine, genome_tools  # noqa: E402

PEAK = 8e12  # bytes per second
T0 = time.perf_counter()


def note(msg):
    sys.stderr.write('[site_time %6.1f s] %s\n' % (time.perf_counter() - T0, msg))
    sys.stderr.flush()


def rate(ms, moved):
    return {'bytes': int(moved), 'GBps': moved / ms / 1e6, 'of_8TBps': moved / (ms * 1e-3) / PEAK}


def pool_of(n, rng):
    pool = np.frombuffer(b'ACGT', np.uint8)[rng.integers(0, 4, n, dtype=np.uint8)]
    for share, run, what in ((0.03, 50, None), (0.02, 10, ord('-')), (0.005, 1, ord('N'))):
        for at in rng.integers(0, n - run, int(n * share / run)).tolist():
            pool[at:at + run] = pool[at:at + run] | 0x20 if what is None else what
    return pool


def synth(n_rows, n_sites, seed):
    """(FASTA text as a uint8 array, the rows' offsets in it)"""
    rng = np.random.default_rng(seed)
    pool = pool_of(min(n_sites, 1 << 26) + (1 << 20), rng)
    heads = [b'>r%d\n' % r for r in range(n_rows)]
    text = np.empty(sum(len(h) for h in heads) + n_rows * (n_sites + 1), np.uint8)
    starts = rng.integers(0, 1 << 20, n_rows).tolist()
    at, where = 0, []
    for r in range(n_rows):
        h = heads[r]
        text[at:at + len(h)] = np.frombuffer(h, np.uint8)
        at += len(h)
        where.append(at)
        done, src = 0, starts[r]
        while done < n_sites:  # the pool again from its start when a row outruns it
            n = min(n_sites - done, len(pool) - src)
            text[at + done:at + done + n] = pool[src:src + n]
            done, src = done + n, 0
        at += n_sites
        text[at] = 10
        at += 1
    assert at == len(text)
    return text, np.array(where, np.int64)


def same_text(path, want):
    """the file at ``path`` holds the bytes ``want``, or the first difference is shown"""
    got = np.memmap(path, np.uint8, 'r') if os.path.getsize(path) else np.zeros(0, np.uint8)
    n = min(len(got), len(want))
    for lo in range(0, n, 1 << 28):
        hi = min(n, lo + (1 << 28))
        bad = np.flatnonzero(got[lo:hi] != want[lo:hi])
        if len(bad):
            at = lo + int(bad[0])
            raise AssertionError('the CLI text (%d bytes) differs from the in-process text (%d) at '
                                 'byte %d: %r / %r' % (len(got), len(want), at,
                                                       got[max(0, at - 60):at + 60].tobytes(),
                                                       want[max(0, at - 60):at + 60].tobytes()))
    assert len(got) == len(want), (len(got), len(want))


def measure(tag, n_rows, n_sites, a, tmp):
    res = {'rows': n_rows, 'sites': n_sites, 'cells': n_rows * n_sites}
    note('%s: making %d x %d' % (tag, n_rows, n_sites))
    text, where = synth(n_rows, n_sites, a.seed)
    res['fasta_bytes'] = int(len(text))

    note('%s: read, upload and pack' % tag)
    walls = []
    for k in range(2):
        t = time.perf_counter()
        dev = engine.FastaGenome.load(text)
        dev.ctx.sync()
        walls.append(time.perf_counter() - t)
        if k == 0:
            dev.close()
    res['load_wall_s'] = walls
    assert len(dev.names) == n_rows and int(dev.lengths.min()) == n_sites

    note('%s: the pass' % tag)
    sites = engine.SiteCounts(dev)
    sites.time(a.warmup)
    ms = [sites.time(a.iters) for _ in range(3)]
    nib = 0.5 * n_rows * n_sites
    res['pass_ms'] = ms
    res['pass_nibble_read'] = rate(min(ms), nib)
    res['pass_all_bytes'] = rate(min(ms), nib + 16 * n_sites)
    res['strips'] = -(-n_rows // engine.SiteCounts.rows_per_strip())
    t = time.perf_counter()
    counts = sites.counts()
    res['execute_and_fetch_wall_s'] = time.perf_counter() - t
    sites.close()
    dev.close()

    note('%s: checking seeded columns' % tag)
    n_cols = max(50, min(4000, 50000000 // n_rows))
    cols = np.unique(np.concatenate([np.random.default_rng(a.seed + 1).integers(0, n_sites, n_cols),
                                     [0, n_sites - 1]]))
    cells = text[where[:, None] + cols[None, :]]
    assert np.array_equal(counts[cols], se.counts_of(cells, len(cols))), tag
    res['checked_columns'] = int(len(cols))

    note('%s: the renderer' % tag)
    t = time.perf_counter()
    out = engine.render_composition(counts)
    res['render_wall_s'] = time.perf_counter() - t
    res['output_bytes'] = int(len(out))
    del counts

    note('%s: the host loop on a sample' % tag)
    s_rows = min(n_rows, max(16, a.sample_cells // 3000))
    s_sites = max(1, min(n_sites, a.sample_cells // s_rows))
    sample = os.path.join(tmp, 'sample.fa')
    with open(sample, 'wb') as fh:
        for r in range(s_rows):
            fh.write(b'>r%d\n' % r)
            fh.write(text[where[r]:where[r] + s_sites].tobytes() + b'\n')
    with open(os.devnull, 'w') as null, contextlib.redirect_stdout(null):
        t = time.perf_counter()
        genome_tools.composition_by_site(sample, native='False')
        loop_s = time.perf_counter() - t
    assert genome_tools.composition_by_site.last_path[1] == 'host'
    res['host_loop'] = {'sample_rows': s_rows, 'sample_sites': s_sites, 'sample_wall_s': loop_s,
                        'extrapolated_s': loop_s / (s_rows * s_sites) * n_rows * n_sites,
                        'note': "the whole alignment at the sample's rate per cell: an "
                                'extrapolation, not a measurement'}

    note('%s: the CLI call in a process of its own' % tag)
    path = os.path.join(tmp, 'aln.fa')
    with open(path, 'wb') as fh:
        fh.write(memoryview(text))
    del text
    env = dict(os.environ, MAGOT_CLI_TIMING='1',
               PYTHONPATH=ROOT + os.pathsep + os.environ.get('PYTHONPATH', ''))
    out_path = os.path.join(tmp, 'out.txt')
    with open(out_path, 'wb') as fh:
        t = time.perf_counter()
        child = subprocess.run([sys.executable, '-m', 'magot_amd.genome_tools',
                                'composition_by_site', path],
                               stdout=fh, stderr=subprocess.PIPE, env=env)
        wall = time.perf_counter() - t
    assert child.returncode == 0, child.stderr[-2000:]
    clock = json.loads(child.stderr.decode().strip().splitlines()[-1])
    assert 'kernels' in clock['cli_phases_s']
    same_text(out_path, out)
    res['cli_native'] = {'wall_s': wall, 'phases_s': clock['cli_phases_s'],
                         'total_s': clock['cli_total_s']}
    os.remove(path)
    os.remove(out_path)
    return res


def shape(text):
    rows, sites = text.lower().split('x')
    return int(rows), int(sites)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--tall', type=shape, default=(100000, 30000))
    ap.add_argument('--wide', type=shape, default=(16, 200000000))
    ap.add_argument('--only', choices=('tall', 'wide'))
    ap.add_argument('--iters', type=int, default=20)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--sample-cells', type=int, default=3000000)
    ap.add_argument('--seed', type=int, default=20261020)
    ap.add_argument('--dir')
    ap.add_argument('--out')
    a = ap.parse_args()
    res = {'iters': a.iters, 'warmup': a.warmup, 'seed': a.seed,
           'shape': {'sites_per_lane': engine.SiteCounts.sites_per_lane(),
                     'sites_per_tile': engine.SiteCounts.sites_per_tile(),
                     'rows_per_strip': engine.SiteCounts.rows_per_strip(),
                     'widening_periods': list(engine.SiteCounts.widening_periods())}}
    with tempfile.TemporaryDirectory(dir=a.dir) as tmp:
        for tag, (n_rows, n_sites) in (('tall', a.tall), ('wide', a.wide)):
            if a.only not in (None, tag):
                continue
            res[tag] = measure(tag, n_rows, n_sites, a, tmp)
            doc = json.dumps(res, indent=1, sort_keys=True)
            if a.out:  # what is measured so far survives a later failure
                with open(a.out, 'w') as fh:
                    fh.write(doc + '\n')
    print(doc)
    return 0


if __name__ == '__main__':
    sys.exit(main())
