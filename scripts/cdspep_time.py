"""Time get_CDS_peptides' device passes against the composed route the library
already had, on a synthetic annotation lowered to one record per CDS.

    python scripts/cdspep_time.py [--config C3] [--n-tx N] [--genome-bases G] [--iters 5]
                                  [--warmup 1] [--rounds 5] [--cli-config small]
                                  [--cli-n-tx 20000] [--cli-genome-bases 40000000] [--dir DIR]
                                  [--out profiles/cdspep_time.json]

The workload is synth.make(config): every CDS interval of every transcript is a
record of its own, '-' ones reverse-complemented.  In this process, with an
event pair around every pass (the *_time entry points):

  * the extraction (engine.ExtractionPlan with OUT_NUC, record order);
  * the fused route: engine.LongestOrfs' calling pass (winners, scan, payload)
    and its text pass;
  * the composed route on the same plan: engine.Orf6Plan (six streams to HBM),
    engine.OrfCalls(longest=True) and its text;
  * a device-to-device copy of as many bytes as the fused passes read and write.

The two routes alternate in ``rounds`` back-to-back rounds; reported are every
round, the medians, the ratio of the medians and the spread (max - min over the
median) of each route.  The fused route reads the extraction's output, the
composed one gathers from the genome itself, so the extraction is reported on
its own and the ratio is given without and with it.  The device memory each
route holds is the drop of free memory across the creation of its handles.
Where no record is flagged both texts must be the same bytes.

Then the whole tool: the CLI call in a fresh child process on files written
under --dir, at ``--cli-config`` (a smaller workload unless asked otherwise: the
FASTA and GTF texts of the large one take minutes to write), wall time.  Needs
a GPU; reads nothing outside the repository.  One JSON document on stdout and
in --out."""

import argparse
import ctypes
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

T0 = time.perf_counter()
CLI_LIMIT_S = 300


def note(msg):
    sys.stderr.write('[cdspep_time %6.1f s] %s\n' % (time.perf_counter() - T0, msg))
    sys.stderr.flush()


_HIP = None


def hip():
    """The HIP runtime libmagot.so already loaded, for the two things the
    library has no entry point for: free memory and a plain device copy."""
    global _HIP
    if _HIP is None:
        _HIP = ctypes.CDLL('libamdhip64.so')
        _HIP.hipMalloc.argtypes = [ctypes.POINTER(ctypes.c_void_p), ctypes.c_size_t]
        _HIP.hipFree.argtypes = [ctypes.c_void_p]
        _HIP.hipMemcpyAsync.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t,
                                        ctypes.c_int, ctypes.c_void_p]
        _HIP.hipEventCreate.argtypes = [ctypes.POINTER(ctypes.c_void_p)]
        _HIP.hipEventRecord.argtypes = [ctypes.c_void_p, ctypes.c_void_p]
        _HIP.hipEventSynchronize.argtypes = [ctypes.c_void_p]
        _HIP.hipEventDestroy.argtypes = [ctypes.c_void_p]
        _HIP.hipEventElapsedTime.argtypes = [ctypes.POINTER(ctypes.c_float), ctypes.c_void_p,
                                             ctypes.c_void_p]
    return _HIP


def hip_ok(rc):
    assert rc == 0, 'HIP error %d' % rc


def free_bytes():
    free, total = ctypes.c_size_t(), ctypes.c_size_t()
    hip_ok(hip().hipMemGetInfo(ctypes.byref(free), ctypes.byref(total)))
    return free.value


def copy_ms(n_bytes, iters):
    """A device-to-device copy that reads and writes n_bytes in all: the mean of
    ``iters`` copies, an event pair around each, as the passes are timed."""
    H = hip()
    half = max(n_bytes // 2, 1)
    a, b, e0, e1 = (ctypes.c_void_p() for _ in range(4))
    hip_ok(H.hipMalloc(ctypes.byref(a), half))
    hip_ok(H.hipMalloc(ctypes.byref(b), half))
    hip_ok(H.hipEventCreate(ctypes.byref(e0)))
    hip_ok(H.hipEventCreate(ctypes.byref(e1)))
    try:
        hip_ok(H.hipMemcpyAsync(b, a, half, 3, None))  # hipMemcpyDeviceToDevice, warm-up
        hip_ok(H.hipDeviceSynchronize())
        total, ms = 0.0, ctypes.c_float()
        for _ in range(iters):
            hip_ok(H.hipEventRecord(e0, None))
            hip_ok(H.hipMemcpyAsync(b, a, half, 3, None))
            hip_ok(H.hipEventRecord(e1, None))
            hip_ok(H.hipEventSynchronize(e1))
            hip_ok(H.hipEventElapsedTime(ctypes.byref(ms), e0, e1))
            total += ms.value
        return total / iters
    finally:
        H.hipEventDestroy(e0)
        H.hipEventDestroy(e1)
        H.hipFree(a)
        H.hipFree(b)


def stats(xs):
    med = float(np.median(xs))
    return {'rounds_ms': [float(x) for x in xs], 'median_ms': med,
            'spread': float((max(xs) - min(xs)) / med) if med else 0.0}


def device_part(a):
    note('making %s' % a.config)
    w = synth.make(a.config, n_tx=a.n_tx, genome_bases=a.genome_bases)
    ex, _ = w.plan_tables()
    n = len(ex)
    tx = np.zeros(n, dtype=engine.TX_DTYPE)
    tx['exon_begin'] = np.arange(n)
    tx['n_exons'] = 1
    res = {'config': a.config, 'records': n, 'cds_bases': int(ex['len'].sum()),
           'transcripts': w.n_tx}
    dev = engine.DeviceGenome(w.contig_views())
    plan = engine.ExtractionPlan(dev, ex, tx, engine.OUT_NUC)
    plan.execute()
    plan.time(a.warmup)
    names = [b'cds%d' % i for i in range(n)]
    note('fused route: create, execute, text')
    f0 = free_bytes()
    lo = engine.LongestOrfs(plan)
    fused_text = lo.text([nm + b'_longestORF' for nm in names])
    res['fused_device_bytes'] = int(f0 - free_bytes())
    flagged = int(np.count_nonzero(lo.flags()))
    res.update(flagged_records=flagged, payload_bytes=lo.payload_bytes,
               text_bytes=len(fused_text), params=lo.params())
    note('composed route: create, execute, text')
    f0 = free_bytes()
    o6 = engine.Orf6Plan(plan)
    o6.execute()
    calls = engine.OrfCalls(o6, longest=True)
    composed_text = calls.text(names)
    res['composed_device_bytes'] = int(f0 - free_bytes())
    res.update(composed_stream_bytes=o6.total, composed_rows=calls.n_orfs)
    none = int(np.count_nonzero(calls.flags() & 1))
    res['composed_none_records'] = none  # the composed route drops these, get_orfs does not
    if not flagged and not none:
        assert fused_text.tobytes() == composed_text.tobytes()
        res['texts_equal'] = True
    else:
        res['texts_equal'] = None
    del fused_text, composed_text
    note('timing, %d rounds' % a.rounds)
    t = {k: [] for k in ('extract', 'fused_call', 'fused_text', 'orf6', 'composed_call',
                         'composed_text')}
    for _ in range(a.rounds):
        t['extract'].append(plan.time(a.iters))
        t['fused_call'].append(lo.time(a.iters))
        t['fused_text'].append(lo.time(a.iters, text=True))
        t['orf6'].append(o6.time(a.iters))
        t['composed_call'].append(calls.time(a.iters))
        t['composed_text'].append(calls.time(a.iters, text=True))
    res['passes'] = {k: stats(v) for k, v in t.items()}
    fused = [x + y for x, y in zip(t['fused_call'], t['fused_text'])]
    fused_x = [x + y for x, y in zip(fused, t['extract'])]
    composed = [x + y + z for x, y, z in zip(t['orf6'], t['composed_call'], t['composed_text'])]
    res['fused'] = stats(fused)
    res['fused_with_extraction'] = stats(fused_x)
    res['composed'] = stats(composed)
    res['composed_over_fused'] = res['composed']['median_ms'] / res['fused']['median_ms']
    res['composed_over_fused_with_extraction'] = (res['composed']['median_ms'] /
                                                  res['fused_with_extraction']['median_ms'])
    moved = 2 * res['cds_bases'] + res['payload_bytes'] + res['text_bytes']
    # what must cross HBM: each of the two passes reads the records once, and the
    # payload and the text are written.  The calling pass loads a record's bytes six
    # times, once per stream; the five reloads are counted as cache hits, not here.
    res['fused_bytes_moved'] = moved
    for obj in (calls, o6, lo, plan, dev):
        obj.close()
    res['copy_same_bytes_ms'] = copy_ms(moved, a.iters)
    return res


def cli_part(a, tmp):
    note('CLI: making %s' % a.cli_config)
    w = synth.make(a.cli_config, n_tx=a.cli_n_tx, genome_bases=a.cli_genome_bases)
    fa, gtf, out = (os.path.join(tmp, x) for x in ('g.fa', 'a.gtf', 'pep.fa'))
    with open(fa, 'w') as fh:
        fh.write(w.fasta_text())
    with open(gtf, 'w') as fh:
        fh.write(w.gtf_text())
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get('PYTHONPATH', ''))
    walls = []
    for _ in range(2):  # the second call finds the files in the page cache
        t = time.perf_counter()
        child = subprocess.run([sys.executable, '-m', 'magot_amd.genome_tools', 'get_CDS_peptides',
                                fa, gtf, out], stderr=subprocess.PIPE, env=env,
                               timeout=CLI_LIMIT_S)
        walls.append(time.perf_counter() - t)
        assert child.returncode == 0, child.stderr[-2000:]
    return {'config': a.cli_config, 'transcripts': w.n_tx, 'cds_intervals': w.n_exons,
            'genome_bases': int(w.contig_len.sum()), 'wall_s': walls,
            'out_bytes': os.path.getsize(out),
            'same_workload_as_device_passes': (a.cli_config, a.cli_n_tx, a.cli_genome_bases) ==
            (a.config, a.n_tx, a.genome_bases)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--config', default='C3')
    ap.add_argument('--n-tx', type=int)
    ap.add_argument('--genome-bases', type=int)
    ap.add_argument('--iters', type=int, default=5)
    ap.add_argument('--warmup', type=int, default=1)
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--cli-config', default='small')
    ap.add_argument('--cli-n-tx', type=int, default=20000)
    ap.add_argument('--cli-genome-bases', type=int, default=40000000)
    ap.add_argument('--dir')
    ap.add_argument('--out')
    a = ap.parse_args()
    res = {'iters': a.iters, 'warmup': a.warmup, 'rounds': a.rounds}
    res['device'] = device_part(a)
    with tempfile.TemporaryDirectory(dir=a.dir) as tmp:
        try:
            res['cli'] = cli_part(a, tmp)
        except (AssertionError, subprocess.TimeoutExpired) as e:  # the device figures stand
            res['cli'] = {'error': repr(e)[:2000]}
    text = json.dumps(res, indent=1, sort_keys=True)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as fh:
            fh.write(text + '\n')
    return 0


if __name__ == '__main__':
    sys.exit(main())
