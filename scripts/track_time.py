"""Time position_dic's device passes on a BASELINE-shaped synthetic (default
C3: 1 Gb) and the whole position_dic call chain on the host.

    python scripts/track_time.py [--config C3] [--iters 20] [--warmup 3]
                                 [--genome-bases N] [--out profiles/track_time_C3.json]

In this process: the genome on the device and a track over it; after a
warm-up, ``iters`` runs of the A/T class pass, the rank directory build, the
window sums at (1000, 1) and (1000, 100), the threshold transitions of each and
one count per contig, an event pair around each (magot_track_time), with the
bytes each moves by its algorithm and that as a fraction of 8 TB/s.  The
yardstick, timed the same way in the same process, is a torch device-to-device
``copy_`` of as many bytes as the class pass moves.  Then
``genome.position_dic``: at_content and sliding_window_calculate (regions at
average >= 0.5, window 1000, jump 100) through the device path, with the share
of packing the genome and of uploading the arrays, and the same calls with
``native=False`` (numpy).  Needs a GPU; reads nothing outside the repository.
One JSON document on stdout and in --out."""

import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from magot_amd import engine, genome, synth  # noqa: E402

PEAK = 8e12  # bytes per second
T0 = time.perf_counter()


def note(msg):
    sys.stderr.write('[track_time %6.1f s] %s\n' % (time.perf_counter() - T0, msg))
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--config', default='C3')
    ap.add_argument('--iters', type=int, default=20)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--genome-bases', type=int)
    ap.add_argument('--n-tx', type=int)
    ap.add_argument('--out')
    a = ap.parse_args()
    note('building the %s synthetic' % a.config)
    w = synth.make(a.config, genome_bases=a.genome_bases, n_tx=a.n_tx)
    contigs = [(nm, seq) for nm, seq in w.contig_views()]
    bases = int(sum(len(s) for _, s in contigs))
    res = {'config': a.config, 'genome_bases': bases, 'contigs': len(contigs), 'iters': a.iters,
           'warmup': a.warmup}
    # torch's runtime first: it finds no device once libmagot has opened one
    dev_span = (bases + 64 + 128 + 31) // 32 * 32
    class_moved = dev_span // 2 + dev_span // 8
    note('timing the copy')
    c_ms = copy_ms(class_moved // 2, a.warmup, a.iters)  # the copy moves twice its size
    res['copy'] = rate(c_ms, class_moved // 2 * 2)
    note('packing the genome')
    dev = engine.DeviceGenome(contigs)
    track = engine.GenomeTrack(dev)
    span = track.n_words * 32
    blocks = (track.n_words + 15) // 16
    plane, directory = span // 8, 4 * (blocks + 1)
    track.base_class()
    passes = {}
    for window, jump in ((1000, 1), (1000, 100)):
        note('windows (%d, %d)' % (window, jump))
        win = track.windows(window, jump)
        s_min = window // 2
        track.time(a.warmup, windows=win, s_min=s_min)
        ms = track.time(a.iters, windows=win, s_min=s_min)
        n = win.n_windows
        flips = len(win.transitions(s_min))
        tag = 'w%d_j%d' % (window, jump)
        passes['windows_' + tag] = dict(rate(ms['windows'], 4 * n + plane + directory), windows=n)
        # count and write each read every sum once
        passes['transitions_' + tag] = dict(rate(ms['transitions'], 8 * n + 12 * ((n + 63) // 64)
                                                 + 8 * flips), transitions=flips, s_min=s_min)
        passes['class'] = rate(ms['class'], span // 2 + span // 8)
        passes['rank'] = rate(ms['rank'], plane + 2 * directory)
        passes['count'] = dict(rate(ms['count'], 16 * len(contigs) + 128 * len(contigs)),
                               rows=len(contigs))
        win.close()
    passes['class']['over_copy_time_per_byte'] = \
        (passes['class']['ms'] / passes['class']['bytes']) / (c_ms / res['copy']['bytes'])
    res['passes'] = passes
    track.close()
    dev.close()

    note('position_dic on the device path')
    seqs = genome.GenomeSequence()
    for nm, seq in contigs:
        dict.__setitem__(seqs, nm, seq.tobytes())
    was, genome.verbose = genome.verbose, False
    try:
        t = time.perf_counter()
        seqs.device()
        pack_s = time.perf_counter() - t
        pd = genome.position_dic(seqs)
        t = time.perf_counter()
        pd.at_content(seqs)
        at_s = time.perf_counter() - t
        assert pd.last_path[1] == 'native', pd.last_path
        t = time.perf_counter()
        up = pd._upload(seqs.device())
        up.ctx.sync()
        upload_s = time.perf_counter() - t
        up.close()
        t = time.perf_counter()
        regions = pd.sliding_window_calculate(1000, 100, operation='average',
                                              output='annotation_set', threshold=0.5)
        win_s = time.perf_counter() - t
        assert pd.last_path[1] == 'native', pd.last_path
        res['position_dic_native'] = {
            'pack_genome_s': pack_s, 'at_content_s': at_s, 'sliding_window_s': win_s,
            'upload_arrays_s': upload_s, 'chain_s': pack_s + at_s + win_s,
            # at_content uploads nothing (the arrays are all zero) and brings every
            # byte back; sliding_window_calculate uploads them once
            'pack_and_upload_share': (pack_s + upload_s) / (pack_s + at_s + win_s),
            'regions': len(regions.region)}
        note('position_dic on the host path')
        hd = genome.position_dic(seqs)
        t = time.perf_counter()
        hd.at_content(seqs, native=False)
        h_at = time.perf_counter() - t
        t = time.perf_counter()
        h_regions = hd.sliding_window_calculate(1000, 100, operation='average',
                                                output='annotation_set', threshold=0.5,
                                                native=False)
        h_win = time.perf_counter() - t
        same = all(np.array_equal(pd[k], hd[k]) for k in pd) and \
            sorted((r.ID, r.coords) for r in regions.region.values()) == \
            sorted((r.ID, r.coords) for r in h_regions.region.values())
        res['position_dic_host'] = {'at_content_s': h_at, 'sliding_window_s': h_win,
                                    'chain_s': h_at + h_win, 'same_results': bool(same)}
    finally:
        genome.verbose = was
    text = json.dumps(res, indent=1, sort_keys=True)
    print(text)
    if a.out:
        with open(a.out, 'w') as fh:
            fh.write(text + '\n')
    return 0


if __name__ == '__main__':
    sys.exit(main())
