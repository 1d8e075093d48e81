"""Time fqstats' device passes and the whole tool on synthetic FASTQ files of
about 1 GB: a short-read shape (every read 150 bases) and a long-read shape
(log-normal lengths, three reads above the dense bound).

    python scripts/fqstats_time.py [--bytes 1000000000] [--iters 20] [--warmup 3]
                                   [--chunk-mb 64] [--shapes short,long] [--dir DIR]
                                   [--out profiles/fqstats_time.json]

Each file (synth.write_fastq) is written under --dir (a temporary directory by
default) and removed after its shape.  In this process: the file parsed into
an engine.ReadLengths (wall time of the upload and every pass), then, after a
warm-up, ``iters`` runs of the line index and the length pass over the chunk
that is still on the device, of the reduction over the whole histogram and of
a device-to-device copy of the chunk's byte count, an event pair around each
(magot_fq_time), with the bytes each moves by its algorithm and that as a
fraction of 8 TB/s.  Then the whole tool: the CLI call in a fresh child
process on the device path and, on the same file, through the host line loop
(``native=False``), and both once more inside this process.  Needs a GPU; reads
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
BLOCK = 4096  # text bytes per block of the line index
T0 = time.perf_counter()


def note(msg):
    sys.stderr.write('[fqstats_time %6.1f s] %s\n' % (time.perf_counter() - T0, msg))
    sys.stderr.flush()


def rate(ms, moved):
    return {'ms': ms, 'bytes': int(moved), 'GBps': moved / ms / 1e6,
            'of_8TBps': moved / (ms * 1e-3) / PEAK}


def tool_s(path, native):
    """wall seconds of one in-process call, its text thrown away"""
    with open(os.devnull, 'w') as null, contextlib.redirect_stdout(null):
        t = time.perf_counter()
        genome_tools.fqstats(path, native=native)
        return time.perf_counter() - t


def child(path, *args):
    """(wall seconds, stdout, the phase clock or None) of the CLI in a fresh process"""
    env = dict(os.environ, MAGOT_CLI_TIMING='1',
               PYTHONPATH=ROOT + os.pathsep + os.environ.get('PYTHONPATH', ''))
    t = time.perf_counter()
    res = subprocess.run([sys.executable, '-m', 'magot_amd.genome_tools', 'fqstats', path] +
                         list(args), stdout=subprocess.PIPE, stderr=subprocess.PIPE, env=env)
    wall = time.perf_counter() - t
    assert res.returncode == 0, res.stderr[-2000:]
    clock = json.loads(res.stderr.decode().strip().splitlines()[-1])
    return wall, res.stdout, clock


def one_shape(shape, a, tmp):
    path = os.path.join(tmp, shape + '.fastq')
    note('writing the %s-read file' % shape)
    dense = engine.ReadLengths().dense
    want = synth.fastq_read_lengths(shape, a.bytes, dense=dense)
    reads, size = synth.write_fastq(path, want)
    res = {'reads': reads, 'file_bytes': size, 'longest': int(want.max()),
           'reads_at_or_above_dense': int((want >= dense).sum())}
    text = genome.read_buffer(path)
    note('parsing')
    t = time.perf_counter()
    r = engine.ReadLengths.parse(text, chunk_bytes=a.chunk_mb << 20)
    first_s = time.perf_counter() - t
    r.close()
    t = time.perf_counter()
    r = engine.ReadLengths.parse(text, chunk_bytes=a.chunk_mb << 20)
    parse_s = time.perf_counter() - t
    assert (r.reads, r.bases) == (reads, int(want.sum())), (r.reads, r.bases)
    res['parse_call'] = {'first_s': first_s, 's': parse_s, 'GBps': size / parse_s / 1e9}
    res['stats'] = r.stats()
    note('timing the passes')
    r.time(a.warmup)
    ms = r.time(a.iters)
    last = ms['chunk_bytes']
    blocks = (last + BLOCK - 1) // BLOCK + 1
    copy = rate(ms['copy'], 2 * last)
    passes = {
        'copy': copy,
        # the text once; 16 bytes per block written, read by the scan, written again
        'line_index': rate(ms['line_index'], last + 48 * blocks),
        # the text once more and a block's prefix; the histogram's atomics are not counted
        'lengths': rate(ms['lengths'], last + 16 * blocks),
        # the bins read, the running totals written and read
        'reduce': rate(ms['reduce'], dense * (8 + 16 + 16)),
    }
    for p in ('line_index', 'lengths'):
        passes[p]['over_copy_time_per_byte'] = \
            (passes[p]['ms'] / passes[p]['bytes']) / (copy['ms'] / copy['bytes'])
    passes['lengths']['ns_per_text_byte'] = ms['lengths'] * 1e6 / last
    res['chunk_bytes'] = last
    res['passes'] = passes
    r.close()
    del text

    note('the CLI call in a process of its own, device path')
    wall, out, clock = child(path)
    res['cli_native'] = {'wall_s': wall, 'phases_s': clock['cli_phases_s'],
                         'total_s': clock['cli_total_s']}
    note('the CLI call in a process of its own, host line loop')
    wall, host_out, clock = child(path, 'native=False')
    assert host_out == out
    res['cli_host'] = {'wall_s': wall, 'total_s': clock['cli_total_s']}
    note('both inside this process')
    native_s = min(tool_s(path, 'True'), tool_s(path, 'True'))
    res['in_process'] = {'native_s': native_s, 'host_s': tool_s(path, 'False')}
    res['output'] = out.decode('latin-1')
    os.remove(path)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--bytes', type=int, default=1_000_000_000)
    ap.add_argument('--iters', type=int, default=20)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--chunk-mb', type=int, default=64)
    ap.add_argument('--shapes', default='short,long')
    ap.add_argument('--dir')
    ap.add_argument('--out')
    a = ap.parse_args()
    res = {'iters': a.iters, 'warmup': a.warmup, 'chunk_mb': a.chunk_mb, 'shapes': {}}
    with tempfile.TemporaryDirectory(dir=a.dir) as tmp:
        for shape in a.shapes.split(','):
            res['shapes'][shape] = one_shape(shape, a, tmp)
    text = json.dumps(res, indent=1, sort_keys=True)
    print(text)
    if a.out:
        with open(a.out, 'w') as fh:
            fh.write(text + '\n')
    return 0


if __name__ == '__main__':
    sys.exit(main())
