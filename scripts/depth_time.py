"""Time depth_from_gff's device passes and the whole tool on a BASELINE-shaped
synthetic (default C2: 100 Mb, one table line per base; --big: C3, 1 Gb).

    python scripts/depth_time.py [--config C2 | --big] [--iters 20] [--warmup 3]
                                 [--chunk-mb 64] [--host-lines 2000000] [--dir DIR]
                                 [--out profiles/depth_time_C2.json]

The table (synth.write_depth_table) and the GFF are written under --dir (a
temporary directory by default).  In this process: the table parsed into an
engine.DepthTrack (wall time of the upload + parse + directory), then, after a
warm-up, ``iters`` runs of the line index and the parse of the chunk that is
still on the device, the directory and one sum per contig, an event pair
around each (magot_depth_time), with the bytes each moves by its algorithm and
that as a fraction of 8 TB/s.  The yardstick, timed the same way in the same
process, is a torch device-to-device ``copy_`` of as many bytes as the parse
pass moves.  Then the whole CLI call in a fresh child process with its phase
clock, and, on a table of about --host-lines lines, the tool with
``native=False`` (the host loop) next to the device path.  Needs a GPU; reads
nothing outside the repository.  One JSON document on stdout and in --out."""

import argparse
import contextlib
import json
import os
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from magot_amd import engine, genome, genome_tools, synth  # noqa: E402

PEAK = 8e12  # bytes per second
T0 = time.perf_counter()


def note(msg):
    sys.stderr.write('[depth_time %6.1f s] %s\n' % (time.perf_counter() - T0, msg))
    sys.stderr.flush()


def copy_ms(n_bytes, warmup, iters):
    import torch
    src = torch.empty(n_bytes, dtype=torch.uint8, device='cuda')
    dst = torch.empty(n_bytes, dtype=torch.uint8, device='cuda')
    src.zero_()
    for _ in range(warmup):
        dst.copy_(src)
    torch.cuda.synchronize()
    total = 0.0
    for _ in range(iters):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        dst.copy_(src)
        b.record()
        b.synchronize()
        total += a.elapsed_time(b)
    del src, dst
    torch.cuda.empty_cache()
    return total / iters


def rate(ms, moved):
    return {'ms': ms, 'bytes': int(moved), 'GBps': moved / ms / 1e6,
            'of_8TBps': moved / (ms * 1e-3) / PEAK}


def synth_files(w, directory, tag):
    """(table path, gff path, lines, table bytes) of a workload"""
    dp = os.path.join(directory, tag + '.depth.txt')
    gp = os.path.join(directory, tag + '.gff')
    lines, size = synth.write_depth_table(dp, w.contig_names, w.contig_len)
    with open(gp, 'w') as fh:
        fh.write(w.gff3_text(ids='ncbi'))
    return dp, gp, lines, size


def tool_s(dp, gp, native):
    """wall seconds of one in-process call, its text thrown away"""
    with open(os.devnull, 'w') as null, contextlib.redirect_stdout(null):
        t = time.perf_counter()
        genome_tools.depth_from_gff(dp, gp, stream_length='1000', native=native)
        return time.perf_counter() - t


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--config', default='C2')
    ap.add_argument('--big', action='store_true', help='C3 (1 Gb, about 20 GB of text)')
    ap.add_argument('--iters', type=int, default=20)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--chunk-mb', type=int, default=64)
    ap.add_argument('--genome-bases', type=int)
    ap.add_argument('--n-tx', type=int)
    ap.add_argument('--host-lines', type=int, default=2_000_000)
    ap.add_argument('--dir')
    ap.add_argument('--out')
    a = ap.parse_args()
    config = 'C3' if a.big else a.config
    with tempfile.TemporaryDirectory(dir=a.dir) as tmp:
        note('writing the %s table' % config)
        w = synth.make(config, genome_bases=a.genome_bases, n_tx=a.n_tx, genome=False)
        dp, gp, lines, size = synth_files(w, tmp, config)
        res = {'config': config, 'lines': lines, 'table_bytes': size, 'contigs': len(w.contig_len),
               'transcripts': w.n_tx, 'iters': a.iters, 'warmup': a.warmup,
               'chunk_bytes': a.chunk_mb << 20}
        text = genome.read_buffer(dp)
        # torch's runtime first: it finds no device once libmagot has opened one
        chunk = min(a.chunk_mb << 20, size)
        chunk_lines = lines * chunk // size
        parse_moved = chunk + 4 * chunk_lines  # the text once, a depth per line
        note('timing the copy')
        c_ms = copy_ms(parse_moved // 2, a.warmup, a.iters)  # the copy moves twice its size
        res['copy'] = rate(c_ms, parse_moved // 2 * 2)
        note('parsing')
        t = time.perf_counter()
        track = engine.DepthTrack.parse(text, chunk_bytes=a.chunk_mb << 20)
        track.ctx.sync()
        first_s = time.perf_counter() - t
        assert track.declined is None, track.declined
        track.close()
        t = time.perf_counter()
        track = engine.DepthTrack.parse(text, chunk_bytes=a.chunk_mb << 20)
        track.ctx.sync()
        parse_s = time.perf_counter() - t
        res['parse_call'] = {'first_s': first_s, 's': parse_s, 'GBps': size / parse_s / 1e9}
        note('timing the passes')
        track.time(a.warmup)
        ms = track.time(a.iters)
        last = ms['chunk_bytes']
        last_lines = lines * last // size
        blocks = (lines + track.block - 1) // track.block
        n = len(track.names)
        passes = {
            'line_index': rate(ms['line_index'], last + 12 * (last // 4096 + 1)),
            'parse': dict(rate(ms['parse'], last + 4 * last_lines), chunk_bytes=last),
            'directory': rate(ms['directory'], 4 * lines + 24 * (blocks + 1)),
            # two directory entries and at most two blocks of depths per row
            'sums': dict(rate(ms['sums'], n * (24 + 16 + 8 * track.block)), rows=n),
        }
        for p in ('line_index', 'parse', 'directory'):
            passes[p]['over_copy_time_per_byte'] = \
                (passes[p]['ms'] / passes[p]['bytes']) / (c_ms / res['copy']['bytes'])
        res['passes'] = passes
        track.close()
        del text

        note('the CLI call in a process of its own')
        env = dict(os.environ, MAGOT_CLI_TIMING='1',
                   PYTHONPATH=ROOT + os.pathsep + os.environ.get('PYTHONPATH', ''))
        t = time.perf_counter()
        child = subprocess.run([sys.executable, '-m', 'magot_amd.genome_tools', 'depth_from_gff',
                                dp, gp], stdout=subprocess.PIPE, stderr=subprocess.PIPE, env=env)
        cli_s = time.perf_counter() - t
        assert child.returncode == 0, child.stderr[-2000:]
        clock = json.loads(child.stderr.decode().strip().splitlines()[-1])
        res['cli'] = {'wall_s': cli_s, 'stdout_bytes': len(child.stdout),
                      'phases_s': clock['cli_phases_s'], 'total_s': clock['cli_total_s']}

        note('the host loop on about %d lines' % a.host_lines)
        small = synth.make(config, genome_bases=a.host_lines,
                           n_tx=max(50, w.n_tx * a.host_lines // max(lines, 1)), genome=False)
        sdp, sgp, s_lines, s_size = synth_files(small, tmp, 'small')
        native_s = tool_s(sdp, sgp, 'True')
        assert genome_tools.depth_from_gff.last_path[1] == 'native', genome_tools.depth_from_gff.last_path
        native_s = min(native_s, tool_s(sdp, sgp, 'True'))
        host_s = tool_s(sdp, sgp, 'False')
        res['host_loop'] = {'lines': s_lines, 'table_bytes': s_size, 'transcripts': small.n_tx,
                            'host_s': host_s, 'native_s': native_s}
    text = json.dumps(res, indent=1, sort_keys=True)
    print(text)
    if a.out:
        with open(a.out, 'w') as fh:
            fh.write(text + '\n')
    return 0


if __name__ == '__main__':
    sys.exit(main())
