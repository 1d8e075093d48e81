"""Time mask_from_gff's device passes on a BASELINE-shaped synthetic (default
C3: 1 Gb, 500 K transcripts) and the whole CLI call in a fresh process.

    python scripts/mask_time.py [--config C3] [--iters 100] [--warmup 10]
                                [--genome-bases N --n-tx T] [--out profiles/mask_time.json]

In this process: the genome on the device, every contig gathered whole, the
mask built from all CDS lines of the synthetic's GFF; after a warm-up,
``iters`` launches of the zeroing + paint kernel and of the text kernel, an
event pair around each (magot_mask_time), with the bytes each moves.  The
yardstick, timed the same way in the same process, is a torch device-to-device
``copy_`` of a buffer of the text's size; the text kernel's time per byte
moved over the copy's is reported beside them.  Then the tool itself
(``python -m magot_amd.genome_tools mask_from_gff``) in a child process on
the same files, its wall time split by the _Clock laps.  Needs a GPU; reads
nothing outside the repository.  One JSON document on stdout and in --out."""

import argparse
import json
import os
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from magot_amd import engine, synth  # noqa: E402


def write_fasta(w, path, width=60):
    with open(path, 'wb') as fh:
        for name, seq in w.contig_views():
            fh.write(b'>' + name.encode('latin-1') + b'\n')
            full = len(seq) // width * width
            lines = np.empty((full // width, width + 1), np.uint8)
            lines[:, :width] = seq[:full].reshape(-1, width)
            lines[:, width] = 10
            fh.write(lines.tobytes())
            if full < len(seq):
                fh.write(seq[full:].tobytes() + b'\n')


T0 = time.perf_counter()


def note(msg):
    sys.stderr.write('[mask_time %6.1f s] %s\n' % (time.perf_counter() - T0, msg))
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
    return total / iters


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--config', default='C3')
    ap.add_argument('--iters', type=int, default=100)
    ap.add_argument('--warmup', type=int, default=10)
    ap.add_argument('--genome-bases', type=int)
    ap.add_argument('--n-tx', type=int)
    ap.add_argument('--out')
    a = ap.parse_args()
    note('building the %s synthetic' % a.config)
    w = synth.make(a.config, genome_bases=a.genome_bases, n_tx=a.n_tx)
    res = {'config': a.config, 'genome_bases': int(w.contig_len.sum()), 'n_tx': w.n_tx,
           'cds_lines': w.n_exons, 'iters': a.iters, 'warmup': a.warmup}
    with tempfile.TemporaryDirectory() as tmp:
        fa, gf = os.path.join(tmp, 'genome.fa'), os.path.join(tmp, 'genes.gff')
        note('writing the FASTA and the GFF')
        write_fasta(w, fa)
        gff = w.gff3_text().encode('latin-1')
        with open(gf, 'wb') as fh:
            fh.write(gff)
        names = list(w.contig_names)
        lengths = [int(x) for x in w.contig_len]
        # torch's runtime first: it finds no device once libmagot has opened one
        note('timing the copy')
        text_bytes = sum(len(nm) + 3 + n for nm, n in zip(names, lengths))
        c_ms = copy_ms(text_bytes, a.warmup, a.iters)
        note('packing the genome, planning, timing')
        dev = engine.DeviceGenome(w.contig_views())
        t = time.perf_counter()
        plan = engine.MaskPlan.build(gff, names, lengths)
        res['gff_scan_s'] = time.perf_counter() - t
        idx = list(range(len(names)))
        ex = engine.whole_contig_plan(dev, idx)
        mask = engine.GenomeMask(ex, plan, idx, names)
        n_pieces = len(plan.intervals)
        covered = int(plan.intervals['len'].astype(np.int64).sum())
        ex.execute()
        mask.execute()
        ex.sync()
        mask.time(a.warmup)
        paint_ms, text_ms = mask.time(a.iters)
        assert text_bytes == mask.text_bytes
        src_bytes = ex.nuc_bytes
        plane_bytes = (src_bytes + 31) // 32 * 4
        # paint: the plane zeroed, the piece table read, the covered words
        # written (edge words read and written by their atomics)
        paint_bytes = plane_bytes + 12 * n_pieces + covered // 8
        # text: source bytes and plane read, text written
        text_moved = src_bytes + plane_bytes + text_bytes
        for obj in (mask, ex, plan, dev):
            obj.close()
        res.update({
            'pieces': n_pieces, 'covered_bases': covered, 'text_bytes': text_bytes,
            'paint_ms': paint_ms, 'paint_bytes': paint_bytes,
            'paint_GBps': paint_bytes / paint_ms / 1e6,
            'text_ms': text_ms, 'text_bytes_moved': text_moved,
            'text_GBps_moved': text_moved / text_ms / 1e6,
            'text_bytes_per_ms': text_bytes / text_ms,
            'copy_ms': c_ms, 'copy_bytes_moved': 2 * text_bytes,
            'copy_GBps_moved': 2 * text_bytes / c_ms / 1e6,
            'text_over_copy_time_per_byte_moved': (text_ms / text_moved) / (c_ms / (2 * text_bytes)),
        })
        # the tool in a process of its own
        note('running the tool')
        env = dict(os.environ, MAGOT_CLI_TIMING='1',
                   PYTHONPATH=ROOT + os.pathsep + os.environ.get('PYTHONPATH', ''))
        with open(os.path.join(tmp, 'masked.fa'), 'wb') as out:
            t = time.perf_counter()
            child = subprocess.run([sys.executable, '-m', 'magot_amd.genome_tools',
                                    'mask_from_gff', fa, gf], stdout=out, stderr=subprocess.PIPE,
                                   env=env, timeout=900)
            res['cli_wall_s'] = time.perf_counter() - t
        if child.returncode != 0:
            sys.stderr.write(child.stderr.decode('latin-1')[-2000:])
            return 1
        res['cli'] = json.loads(child.stderr.decode().strip().splitlines()[-1])
        res['cli_output_bytes'] = os.path.getsize(os.path.join(tmp, 'masked.fa'))
    text = json.dumps(res, indent=1, sort_keys=True)
    print(text)
    if a.out:
        with open(a.out, 'w') as fh:
            fh.write(text + '\n')
    return 0


if __name__ == '__main__':
    sys.exit(main())
