"""Time besthits_from_psl's device passes, its host steps and the whole tool on
a seeded synthetic PSL made in memory.

    python scripts/psl_time.py [--lines 3000000] [--iters 20] [--warmup 3] [--sample 200000]
                               [--long-share 0.02] [--dir DIR] [--out profiles/psl_time.json]

The text: ``--lines`` data lines behind the five-line psLayout header, grouped
by query as BLAT writes them.  Hits per query are 1 + floor(Pareto(1.16)),
capped at 5000: half the queries have one hit, a few have thousands (the
figures of the draw are in the result: 'queries', 'hits_max', 'hits_p50',
'hits_p99').  A share ``--long-share`` of the lines carries block lists of 300
blocks (about 4.9 KB), the others 1 to 8 blocks (about 160 bytes).  At the
defaults the text is about 0.7 GB, beyond the 256 MiB cache.

In this process, on the device: ``warmup`` then ``iters`` runs of each pass with
an event pair around it (magot_psl_time; device ms) and of a device-to-device
copy of the text, with the bytes each pass must move at the least; the upload
inside one parse (device ms from the first copy's enqueue to the last byte's
arrival, the host's staging copies in between); the whole engine.BestHits.parse
call three times (wall time: upload, allocations, passes, three
synchronisations).  On the host (wall time): the Python 2 dict order from the
hashes, the renderer, and the tool's line loop (native='False') on the first
``--sample`` lines, its rate scaled to the whole text marked as an
extrapolation.  Then the whole tool: the CLI call in a fresh child process on
the text written under --dir (wall time, interpreter start and library load
included), and once more inside this one.  Needs a GPU; reads nothing outside
the repository.  One JSON document on stdout and in --out."""

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

from magot_amd import engine, genome_tools  # noqa: E402

PEAK = 8e12  # bytes per second
T0 = time.perf_counter()
HEADER = (b'psLayout version 3\n\nmatch\tmis- \trep. \tN\'s\tQ gap\tQ gap\tT gap\tT gap\tstrand\t'
          b'Q   \tQ   \tQ    \tQ  \tT   \tT   \tT    \tT  \tblock\tblockSizes \tqStarts\t tStarts\n'
          b'     \tmatch\tmatch\t   \tcount\tbases\tcount\tbases\t      \tname\tsize\tstart\tend\t'
          b'name\tsize\tstart\tend\tcount\n' + b'-' * 159 + b'\n')


def note(msg):
    sys.stderr.write('[psl_time %6.1f s] %s\n' % (time.perf_counter() - T0, msg))
    sys.stderr.flush()


def rate(ms, moved):
    return {'ms': ms, 'bytes': int(moved), 'GBps': moved / ms / 1e6 if ms else None,
            'of_8TBps': moved / (ms * 1e-3) / PEAK if ms else None}


def synth_psl(n_lines, long_share, seed):
    """(text, shape): the PSL described above"""
    rng = np.random.default_rng(seed)
    hits = np.minimum(1 + np.floor(rng.pareto(1.16, n_lines)).astype(np.int64), 5000)
    n_q = int(np.searchsorted(np.cumsum(hits), n_lines)) + 1
    hits = hits[:n_q]
    hits[-1] -= int(hits.sum()) - n_lines
    query = np.repeat(np.arange(n_q), hits)
    m = rng.integers(40, 1500, n_lines)
    mm = rng.integers(0, 40, n_lines)
    blocks = np.where(rng.random(n_lines) < long_share, 300, rng.integers(1, 9, n_lines))
    start = rng.integers(0, 90000000, n_lines)
    lists = {b: (''.join('%d,' % (30 + j % 70) for j in range(b)),
                 ''.join('%d,' % (40 * j) for j in range(b)),
                 ''.join('%d,' % (1000000 + 45 * j) for j in range(b)))
             for b in list(range(1, 9)) + [300]}
    row = '%d\t%d\t0\t0\t1\t12\t2\t340\t%s\tread_%07d/ccs\t%d\t0\t%d\tchr%d\t158000000\t%d\t%d\t%d\t%s\t%s\t%s\n'
    parts = [HEADER.decode('latin-1')]
    for q, a, b, k, s in zip(query.tolist(), m.tolist(), mm.tolist(), blocks.tolist(),
                             start.tolist()):
        sizes, qs, ts = lists[k]
        parts.append(row % (a, b, '+-'[s & 1], q, a + b + 12, a + b, 1 + s % 29, s, s + a + b + 340,
                            k, sizes, qs, ts))
    text = ''.join(parts).encode('latin-1')
    shape = {'lines': n_lines + 5, 'data_lines': n_lines, 'bytes': len(text), 'queries': n_q,
             'hits_max': int(hits.max()), 'hits_p50': float(np.percentile(hits, 50)),
             'hits_p99': float(np.percentile(hits, 99)), 'hits_mean': n_lines / n_q,
             'long_lines': int((blocks == 300).sum()), 'long_share': long_share, 'seed': seed,
             'order': 'grouped by query'}
    return text, shape


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--lines', type=int, default=3000000)
    ap.add_argument('--long-share', type=float, default=0.02)
    ap.add_argument('--iters', type=int, default=20)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--sample', type=int, default=200000)
    ap.add_argument('--seed', type=int, default=20261020)
    ap.add_argument('--dir')
    ap.add_argument('--out')
    a = ap.parse_args()
    res = {'iters': a.iters, 'warmup': a.warmup}
    note('making the text')
    text, res['text'] = synth_psl(a.lines, a.long_share, a.seed)
    n, L = len(text), res['text']['lines']

    note('parse: warm-up, then three calls')
    hits = engine.BestHits.parse(text)
    assert isinstance(hits, engine.BestHits), hits
    hits.close()
    walls, uploads = [], []
    for _ in range(3):
        t = time.perf_counter()
        hits = engine.BestHits.parse(text)
        hits.ctx.sync()
        walls.append(time.perf_counter() - t)
        uploads.append(hits.upload_ms)
        if _ < 2:
            hits.close()
    assert (hits.n_data, hits.n_groups, hits.n_lines) == (a.lines, res['text']['queries'], L)
    res['parse_call_wall_s'] = walls
    res['upload_device_ms'] = uploads
    res['upload_GBps'] = [n / ms / 1e6 for ms in uploads]

    note('timing the passes')
    hits.time(a.warmup)
    ms = hits.time(a.iters)
    D, G = hits.n_data, hits.n_groups
    copy = rate(ms['copy'], 2 * n)
    res['passes'] = {
        'copy': copy,
        # the text read twice (count, fill), a line start written per line
        'line_index': rate(ms['line_index'], 2 * n + 8 * L),
        # the lines' heads up to the 10th tab are read, not the text: at the least
        # the index entry read and 29 bytes written per line
        'parse': rate(ms['parse'], L * (16 + 29)),
        'compact': rate(ms['compact'], L * (4 + 4 + 4 + 16 + 16)),
        # at least one read and one write of 16 bytes per pair
        'sort': rate(ms['sort'], 2 * 16 * D),
        'verify': rate(ms['verify'], 16 * D),
        'reduce': rate(ms['reduce'], 16 * D + 24 * G),
        'order': rate(ms['order'], G * (8 + 2 * 8 + 16 + 40)),
    }
    res['passes']['device_total_ms'] = sum(ms[k] for k in engine.BestHits.PASSES if k != 'copy')
    res['passes']['parse']['ns_per_line'] = ms['parse'] * 1e6 / L
    res['passes']['sort']['over_copy_time_per_byte'] = \
        (ms['sort'] / (2 * 16 * D)) / (copy['ms'] / copy['bytes'])

    note('the host order and the renderer')
    g = hits.groups()
    p_off, p_len = hits.pass_lines()
    order_s, render_s = [], []
    for _ in range(3):
        t = time.perf_counter()
        perm = engine.py2_order_of_hashes(g['hash'])
        order_s.append(time.perf_counter() - t)
        off = np.concatenate([p_off, g['off'][perm]])
        length = np.concatenate([p_len, g['len'][perm]])
        t = time.perf_counter()
        out = engine.render_lines(text, off, length)
        render_s.append(time.perf_counter() - t)
    res['host_order_wall_s'], res['host_render_wall_s'] = order_s, render_s
    res['output_bytes'] = int(len(out))
    hits.close()

    with tempfile.TemporaryDirectory(dir=a.dir) as tmp:
        note('the line loop on a sample')
        cut = 0
        for _ in range(a.sample + 5):
            cut = text.index(b'\n', cut) + 1
        sample_path = os.path.join(tmp, 'sample.psl')
        with open(sample_path, 'wb') as fh:
            fh.write(text[:cut])
        with open(os.devnull, 'w') as null, contextlib.redirect_stdout(null):
            t = time.perf_counter()
            genome_tools.besthits_from_psl(sample_path, native='False')
            loop_s = time.perf_counter() - t
        assert genome_tools.besthits_from_psl.last_path[1] == 'host'
        res['line_loop'] = {'sample_lines': a.sample + 5, 'sample_bytes': cut, 'sample_wall_s': loop_s,
                            'extrapolated_s': loop_s / (a.sample + 5) * L,
                            'note': 'the whole text at the sample\'s rate per line: an '
                                    'extrapolation, not a measurement'}

        note('the CLI call in a process of its own')
        path = os.path.join(tmp, 'hits.psl')
        with open(path, 'wb') as fh:
            fh.write(text)
        env = dict(os.environ, MAGOT_CLI_TIMING='1',
                   PYTHONPATH=ROOT + os.pathsep + os.environ.get('PYTHONPATH', ''))
        out_path = os.path.join(tmp, 'best.psl')
        with open(out_path, 'wb') as fh:
            t = time.perf_counter()
            child = subprocess.run([sys.executable, '-m', 'magot_amd.genome_tools',
                                    'besthits_from_psl', path],
                                   stdout=fh, stderr=subprocess.PIPE, env=env)
            wall = time.perf_counter() - t
        assert child.returncode == 0, child.stderr[-2000:]
        clock = json.loads(child.stderr.decode().strip().splitlines()[-1])
        assert os.path.getsize(out_path) == res['output_bytes']
        res['cli_native'] = {'wall_s': wall, 'phases_s': clock['cli_phases_s'],
                             'total_s': clock['cli_total_s']}
        note('once more inside this process')
        with open(os.devnull, 'w') as null, contextlib.redirect_stdout(null):
            t = time.perf_counter()
            genome_tools.besthits_from_psl(path)
            res['in_process_wall_s'] = time.perf_counter() - t
        assert genome_tools.besthits_from_psl.last_path[1] == 'native'
    doc = json.dumps(res, indent=1, sort_keys=True)
    print(doc)
    if a.out:
        with open(a.out, 'w') as fh:
            fh.write(doc + '\n')
    return 0


if __name__ == '__main__':
    sys.exit(main())
