"""Time purge_overlaps' device passes and the whole tool on the C3 synthetic
annotation purged against a seeded set of repeat intervals.

    python scripts/overlap_time.py [--config C3] [--iters 20] [--warmup 3] [--sample 200]
                                   [--dir DIR] [--out profiles/overlap_time.json]

The second file is the workload's annotation in coordinate order (synth.make,
order='sorted'): a gene, an mRNA and its CDS lines per transcript, about 5 M
lines for C3.  The first file is a repeat track drawn by the synthetic
soft-mask model (alternating gaps and runs of geometric lengths, runs of 300
bases on average over 40 % of every contig): about 1.3 M lines for C3.  Both are
written under --dir (a temporary directory by default) and removed at the end.

In this process: the host planner over both files (wall time), the index build
and one purge query (wall time of the calls, uploads and downloads included),
then, after a warm-up, ``iters`` runs of each device pass with an event pair
around it (magot_overlap_time) and of a device-to-device copy of the sorted
tables, with the bytes each pass must move at the least.  On the same host, at
full size, numpy's ``sort`` + ``searchsorted`` restatement of the same searches
(its flags must equal the device's), and the reference's pair loop restated
over the first --sample lines of the second file that have a seqid of the first,
with its time scaled to every pair of the two files: that figure is an
extrapolation, not a measurement.  Then the whole tool: the CLI call in a
fresh child process and once more inside this one.  Needs a GPU; reads nothing
outside the repository.  One JSON document on stdout and in --out."""

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

from magot_amd import engine, genome_tools, synth  # noqa: E402

PEAK = 8e12  # bytes per second
T0 = time.perf_counter()


def note(msg):
    sys.stderr.write('[overlap_time %6.1f s] %s\n' % (time.perf_counter() - T0, msg))
    sys.stderr.flush()


def rate(ms, moved):
    return {'ms': ms, 'bytes': int(moved), 'GBps': moved / ms / 1e6 if ms else None,
            'of_8TBps': moved / (ms * 1e-3) / PEAK if ms else None}


def write_annotation(path, w):
    """gene, mRNA and CDS lines of every transcript, as Workload.gff3_text
    writes them; returns the line count"""
    first = np.concatenate([[0], np.cumsum(w.ex_count)])
    n = 0
    with open(path, 'w') as fh:
        fh.write('##gff-version 3\n')
        for t in range(w.n_tx):
            c = w.contig_names[w.tx_contig[t]]
            st = '+' if w.tx_strand[t] > 0 else '-'
            a, b = first[t], first[t + 1]
            lo, hi = int(w.ex_start[a]) + 1, int(w.ex_start[b - 1] + w.ex_len[b - 1])
            lines = ['%s\tsynth\tgene\t%d\t%d\t.\t%s\t.\tID=gene%d;Name=G%d\n' % (c, lo, hi, st, t, t),
                     '%s\tsynth\tmRNA\t%d\t%d\t.\t%s\t.\tID=rna%d;Parent=gene%d\n'
                     % (c, lo, hi, st, t, t)]
            for e in range(a, b):
                s0 = int(w.ex_start[e])
                lines.append('%s\tsynth\tCDS\t%d\t%d\t.\t%s\t0\tID=cds%d;Parent=rna%d\n'
                             % (c, s0 + 1, s0 + int(w.ex_len[e]), st, t, t))
            fh.write(''.join(lines))
            n += len(lines)
    return n + 1


def write_repeats(path, w, seed, frac=0.4, mean=300.0):
    """The repeat track: per contig alternating gaps and runs of geometric
    lengths; returns (line count, bases covered)"""
    rng = np.random.default_rng(seed)
    gap_mean = mean * (1.0 - frac) / frac
    n = covered = 0
    with open(path, 'w') as fh:
        for name, length in zip(w.contig_names, w.contig_len.tolist()):
            k = int(length / (mean + gap_mean) * 1.2) + 16
            gaps, runs = rng.geometric(1.0 / gap_mean, k), rng.geometric(1.0 / mean, k)
            ends = np.cumsum(gaps + runs)
            starts = ends - runs + 1  # 1-based, closed
            keep = ends <= length
            starts, ends = starts[keep], ends[keep]
            fh.write(''.join('%s\tsynth\trepeat\t%d\t%d\t.\t+\t.\tID=r%d\n' % (name, a, b, n + i)
                             for i, (a, b) in enumerate(zip(starts.tolist(), ends.tolist()))))
            n += len(starts)
            covered += int((ends - starts + 1).sum())
    return n, covered


def numpy_flags(index, query, n_seq):
    """purge's three tests by sort + searchsorted per seqid, as the device runs them"""
    iseq, p0, p1 = index
    qseq, c0, c1 = query
    out = np.zeros(len(qseq), bool)
    for s in range(n_seq):
        m = iseq == s
        q = np.flatnonzero(qseq == s)
        if not m.any() or not len(q):
            continue
        a0, a1, x0, x1 = p0[m], p1[m], c0[q], c1[q]
        inner = a0 < a1
        in_s, in_e, all_s = np.sort(a0[inner]), np.sort(a1[inner]), np.sort(a0)
        hit = np.searchsorted(in_s, x0, 'left') > np.searchsorted(in_e, x0, 'right')
        hit |= np.searchsorted(in_s, x1, 'left') > np.searchsorted(in_e, x1, 'right')
        hit |= (x0 < x1) & (np.searchsorted(all_s, x1, 'left') > np.searchsorted(all_s, x0, 'right'))
        out[q] = hit
    return out


def pair_loop(index, query, sample):
    """(seconds, pairs tested, flags) of the reference's loop over every pair,
    for the first ``sample`` queries"""
    by_seq = {}
    for s, a, b in zip(*(x.tolist() for x in index)):
        by_seq.setdefault(s, []).append([a, b])
    rows = list(zip(*(x[:sample].tolist() for x in query)))
    flags, pairs = [], 0
    t = time.perf_counter()
    for s, c0, c1 in rows:
        printline = True
        for purge_coords in by_seq.get(s, ()):
            if (purge_coords[0] < c0 < purge_coords[1] or purge_coords[0] < c1 < purge_coords[1] or
                    c0 < purge_coords[0] < c1):
                printline = False
                continue
        pairs += len(by_seq.get(s, ()))
        flags.append(not printline)
    return time.perf_counter() - t, pairs, np.asarray(flags, bool)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--config', default='C3')
    ap.add_argument('--tx', type=int, help='rescale the workload (rehearsals)')
    ap.add_argument('--genome-bases', type=int)
    ap.add_argument('--iters', type=int, default=20)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--sample', type=int, default=200)
    ap.add_argument('--dir')
    ap.add_argument('--out')
    a = ap.parse_args()
    res = {'config': a.config, 'iters': a.iters, 'warmup': a.warmup}
    with tempfile.TemporaryDirectory(dir=a.dir) as tmp:
        first, second = os.path.join(tmp, 'repeats.gff'), os.path.join(tmp, 'annotation.gff')
        note('building the workload tables')
        w = synth.make(a.config, order='sorted', genome=False, n_tx=a.tx,
                       genome_bases=a.genome_bases)
        note('writing the annotation')
        lines2 = write_annotation(second, w)
        note('writing the repeat track')
        lines1, covered = write_repeats(first, w, synth.SEED_BASE + 40)
        total = int(w.contig_len.sum())
        res['files'] = {'first_lines': lines1, 'first_bytes': os.path.getsize(first),
                        'second_lines': lines2, 'second_bytes': os.path.getsize(second),
                        'contigs': len(w.contig_len), 'genome_bases': total,
                        'repeat_fraction': covered / total}

        note('the host planner')
        b1, b2 = genome_tools._map_file(first), genome_tools._map_file(second)
        t = time.perf_counter()
        plan, why = engine.OverlapPlan.build(b1, b2)
        res['planner_s'] = time.perf_counter() - t
        assert plan is not None, why
        t0, t1 = plan.tables
        rows = np.flatnonzero(t0['flag'])
        index = tuple(np.ascontiguousarray(t0[c][rows]).astype(np.int64) for c in ('seq', 'c0', 'c1'))
        asked = np.flatnonzero(t1['seq'] != 0xffffffff)
        query = tuple(np.ascontiguousarray(t1[c][asked]).astype(np.int64)
                      for c in ('seq', 'c0', 'c1'))
        n, nq = len(rows), len(asked)
        res['intervals'], res['queries'], res['seqids'] = n, nq, plan.n_seq
        flagged = int(t1['flag'].sum())  # the lines that can be printed at all

        note('the index and one query')
        t = time.perf_counter()
        ix = engine.IntervalIndex(*index, n_seq=plan.n_seq)
        ix.ctx.sync()
        res['index_call_s'] = time.perf_counter() - t
        t = time.perf_counter()
        flags = ix.purge_flags(*query)
        res['purge_call_s'] = time.perf_counter() - t
        res['dropped'] = int(flags.sum())
        ix.overlap_counts(*query)  # the same query set, for the overlap pass
        note('timing the passes')
        ix.time(a.warmup)
        ms = ix.time(a.iters)
        ix.close()
        copy = rate(ms['copy'], 2 * ms['copy_bytes'])
        segs = 3 * (plan.n_seq + 1)
        res['passes'] = {
            'copy': copy,
            # the intervals read, five keys and the end written per interval
            'keys': rate(ms['keys'], n * (20 + 48)),
            # per table and per radix pass at least one read and one write; the
            # least any sort can do is one of each
            'sort': rate(ms['sort'], 2 * 6 * 8 * n),
            'segments': rate(ms['segments'], 8 * segs),
            # the query read, one byte written; the searched keys are not counted
            'purge': rate(ms['purge'], nq * (20 + 1)),
            'overlap': rate(ms['overlap'], nq * (20 + 8)),
        }
        res['passes']['build_ms'] = ms['keys'] + ms['sort'] + ms['segments']
        res['passes']['sort']['over_copy_time_per_byte'] = \
            (ms['sort'] / (2 * 6 * 8 * n)) / (copy['ms'] / copy['bytes'])
        res['passes']['purge']['ns_per_query'] = ms['purge'] * 1e6 / max(nq, 1)
        res['passes']['overlap']['ns_per_query'] = ms['overlap'] * 1e6 / max(nq, 1)

        note('numpy sort + searchsorted at full size')
        t = time.perf_counter()
        host = numpy_flags(index, query, plan.n_seq)
        res['numpy_s'] = time.perf_counter() - t
        assert np.array_equal(host, flags), int((host != flags).sum())

        note('the pair loop on a sample')
        loop_s, pairs, loop_flags = pair_loop(index, query, a.sample)
        assert np.array_equal(loop_flags, flags[:a.sample])
        per_seq_i = np.bincount(index[0], minlength=plan.n_seq)
        all_pairs = int(per_seq_i[query[0]].sum())
        res['pair_loop'] = {'sample_queries': min(a.sample, nq), 'sample_pairs': pairs,
                            'sample_s': loop_s, 'all_pairs': all_pairs,
                            'extrapolated_s': loop_s / max(pairs, 1) * all_pairs,
                            'note': 'extrapolated from the sample; not a measurement'}
        plan.close()
        del b1, b2, t0, t1

        note('the CLI call in a process of its own')
        env = dict(os.environ, MAGOT_CLI_TIMING='1',
                   PYTHONPATH=ROOT + os.pathsep + os.environ.get('PYTHONPATH', ''))
        out_path = os.path.join(tmp, 'purged.gff')
        with open(out_path, 'wb') as out:
            t = time.perf_counter()
            child = subprocess.run([sys.executable, '-m', 'magot_amd.genome_tools',
                                    'purge_overlaps', first, second],
                                   stdout=out, stderr=subprocess.PIPE, env=env)
            wall = time.perf_counter() - t
        assert child.returncode == 0, child.stderr[-2000:]
        clock = json.loads(child.stderr.decode().strip().splitlines()[-1])
        with open(out_path, 'rb') as fh:
            kept = sum(chunk.count(b'\n') for chunk in iter(lambda: fh.read(1 << 24), b''))
        assert kept == flagged - res['dropped'], (kept, flagged, res['dropped'])
        res['cli_native'] = {'wall_s': wall, 'phases_s': clock['cli_phases_s'],
                             'total_s': clock['cli_total_s'], 'lines_kept': kept,
                             'output_bytes': os.path.getsize(out_path)}
        note('once more inside this process')
        with open(os.devnull, 'w') as null, contextlib.redirect_stdout(null):
            t = time.perf_counter()
            genome_tools.purge_overlaps(first, second)
            res['in_process_s'] = time.perf_counter() - t
        assert genome_tools.purge_overlaps.last_path[1] == 'native'
    text = json.dumps(res, indent=1, sort_keys=True)
    print(text)
    if a.out:
        with open(a.out, 'w') as fh:
            fh.write(text + '\n')
    return 0


if __name__ == '__main__':
    sys.exit(main())
