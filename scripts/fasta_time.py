"""Time exclude_from_fasta's and fasta2tab's device passes, their host steps and
the whole tools on two seeded synthetic FASTA files made in memory.

    python scripts/fasta_time.py [--records 2000000] [--names 200000] [--contigs 24]
                                 [--contig-mb 40] [--iters 10] [--warmup 2] [--dir DIR]
                                 [--out profiles/fasta_time.json]

'transcriptome': ``--records`` records with Trinity-style headers (a first
word and a description) and sequences of 200 to 1200 bases in lines of 60;
``--names`` of the first words, drawn without order, are the exclusion list,
compared with just_firstword=True.  'genome': ``--contigs`` records of
``--contig-mb`` million bases each on ONE line (the long-line path), two of
them excluded by name.

Per file, in this process, on the device: the upload inside one parse (device
ms), the whole engine.FastaRecords.parse call three times (wall), ``warmup``
then ``iters`` runs of each pass with an event pair around it
(magot_fastarec_time; device ms), the reflow's time per byte over the plain
device copy's, and the exclude and render calls (wall, their transfers
included).  On the host (wall): the Python 2 dict order from the hashes, and
the tool's host loop (native='False') on the whole file -- its size is in the
result.  Then the whole tools: each CLI call in a fresh child process on the
file written under --dir (wall, interpreter start and library load included).
Needs a GPU; reads nothing outside the repository.  One JSON document on stdout
and in --out."""

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

T0 = time.perf_counter()


def note(msg):
    sys.stderr.write('[fasta_time %6.1f s] %s\n' % (time.perf_counter() - T0, msg))
    sys.stderr.flush()


def transcriptome(n_records, n_names, seed):
    """(text, the exclusion file's bytes, shape)"""
    rng = np.random.default_rng(seed)
    pool = rng.choice(np.frombuffer(b'ACGT', np.uint8), 1 << 22).tobytes()
    lens = rng.integers(200, 1201, n_records).tolist()
    at = rng.integers(0, (1 << 22) - 1300, n_records).tolist()
    parts, words = [], []
    for r, (n, o) in enumerate(zip(lens, at)):
        word = 'TRINITY_DN%d_c%d_g1_i%d' % (r // 3, r % 3, 1 + r % 2)
        words.append(word)
        seq = pool[o:o + n]
        parts.append(b'>%s len=%d path=[%d:0-%d]\n' % (word.encode(), n, o, n - 1))
        parts.append(b'\n'.join(seq[i:i + 60] for i in range(0, n, 60)))
        parts.append(b'\n')
    text = b''.join(parts)
    picked = rng.choice(n_records, min(n_names, n_records), replace=False)
    names = ''.join(words[i] + '\n' for i in picked.tolist()).encode()
    return text, names, {'records': n_records, 'bytes': len(text), 'names': len(picked),
                         'line_bytes': 60, 'seed': seed}


def genome_shape(n_contigs, contig_mb, seed):
    rng = np.random.default_rng(seed)
    block = rng.choice(np.frombuffer(b'ACGTacgtN', np.uint8), contig_mb * 1000000).tobytes()
    parts = []
    for c in range(n_contigs):
        cut = (c * 7919) % 1000
        parts += [b'>chr%d assembled\n' % (c + 1), block[cut:], block[:cut], b'\n']
    text = b''.join(parts)
    names = b'chr2 assembled\nchr%d assembled\n' % n_contigs
    return text, names, {'records': n_contigs, 'bytes': len(text), 'names': 2,
                         'line_bytes': contig_mb * 1000000, 'seed': seed}


def measure(label, text, names, first_word, a, tmp):
    res = {}
    n = len(text)
    note('%s: parse, a warm-up then three calls' % label)
    recs = engine.FastaRecords.parse(text)
    assert isinstance(recs, engine.FastaRecords), recs
    recs.close()
    walls, uploads = [], []
    for k in range(3):
        t = time.perf_counter()
        recs = engine.FastaRecords.parse(text)
        recs.ctx.sync()
        walls.append(time.perf_counter() - t)
        uploads.append(recs.upload_ms)
        if k < 2:
            recs.close()
    res['sizes'] = {'lines': recs.n_lines, 'records': recs.n_records, 'keys': recs.n_keys}
    res['parse_call_wall_s'] = walls
    res['upload_device_ms'] = uploads
    res['upload_GBps'] = [n / ms / 1e6 for ms in uploads]

    note('%s: timing the passes' % label)
    recs.time(a.warmup)
    ms = recs.time(a.iters)
    res['passes_ms'] = {k: ms[k] for k in engine.FastaRecords.PASSES}
    res['device_total_ms'] = sum(ms[k] for k in engine.FastaRecords.PASSES if k != 'copy')
    res['text_bytes'], res['reflow_bytes'] = ms['text_bytes'], ms['reflow_bytes']
    res['copy_GBps_read_plus_write'] = 2 * n / ms['copy'] / 1e6
    res['reflow_GBps_read_plus_write'] = 2 * ms['reflow_bytes'] / ms['reflow'] / 1e6
    res['reflow_over_copy_time_per_byte'] = \
        (ms['reflow'] / ms['reflow_bytes']) / (ms['copy'] / ms['text_bytes'])

    note('%s: membership, order, render' % label)
    listed = names.replace(b'\r', b'').split(b'\n')
    keys = recs.keys()
    member_s, order_s, render_s = [], [], []
    for _ in range(3):
        t = time.perf_counter()
        keep = recs.exclude(listed, first_word=first_word)
        member_s.append(time.perf_counter() - t)
        t = time.perf_counter()
        perm = engine.py2_order_of_hashes(keys['hash'])
        order_s.append(time.perf_counter() - t)
        t = time.perf_counter()
        out = recs.render(keys['last_record'][perm][keep[perm]], 'fasta')
        render_s.append(time.perf_counter() - t)
    res['exclude_call_wall_s'], res['host_order_wall_s'] = member_s, order_s
    res['render_call_wall_s'] = render_s
    res['kept'], res['output_bytes'] = int(keep.sum()), int(len(out))
    recs.close()

    path, list_path = os.path.join(tmp, label + '.fa'), os.path.join(tmp, label + '.txt')
    with open(path, 'wb') as fh:
        fh.write(text)
    with open(list_path, 'wb') as fh:
        fh.write(names)
    flag = 'just_firstword=%s' % first_word
    note('%s: the host loops on the whole file' % label)
    with open(os.devnull, 'w') as null, contextlib.redirect_stdout(null):
        t = time.perf_counter()
        genome_tools.exclude_from_fasta(path, list_path, str(first_word), native='False')
        res['host_exclude'] = {'wall_s': time.perf_counter() - t, 'file_bytes': n,
                               'records': res['sizes']['records'], 'names': len(listed) - 1}
        t = time.perf_counter()
        genome_tools.fasta2tab(path, native='False')
        res['host_fasta2tab'] = {'wall_s': time.perf_counter() - t, 'file_bytes': n}
    env = dict(os.environ, MAGOT_CLI_TIMING='1',
               PYTHONPATH=ROOT + os.pathsep + os.environ.get('PYTHONPATH', ''))
    for tool, argv in (('exclude_from_fasta', [path, list_path, flag]), ('fasta2tab', [path])):
        note('%s: %s in a process of its own' % (label, tool))
        out_path = os.path.join(tmp, 'out.txt')
        with open(out_path, 'wb') as fh:
            t = time.perf_counter()
            child = subprocess.run([sys.executable, '-m', 'magot_amd.genome_tools', tool] + argv,
                                   stdout=fh, stderr=subprocess.PIPE, env=env)
            wall = time.perf_counter() - t
        assert child.returncode == 0, child.stderr[-2000:]
        clock = json.loads(child.stderr.decode().strip().splitlines()[-1])
        size = os.path.getsize(out_path)
        assert size == (res['output_bytes'] if tool == 'exclude_from_fasta' else ms['reflow_bytes'])
        res['cli_' + tool] = {'wall_s': wall, 'phases_s': clock['cli_phases_s'],
                              'total_s': clock['cli_total_s'], 'output_bytes': size}
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--records', type=int, default=2000000)
    ap.add_argument('--names', type=int, default=200000)
    ap.add_argument('--contigs', type=int, default=24)
    ap.add_argument('--contig-mb', type=int, default=40)
    ap.add_argument('--iters', type=int, default=10)
    ap.add_argument('--warmup', type=int, default=2)
    ap.add_argument('--seed', type=int, default=20261020)
    ap.add_argument('--dir')
    ap.add_argument('--out')
    a = ap.parse_args()
    res = {'iters': a.iters, 'warmup': a.warmup, 'params': engine.FastaRecords.params()}
    with tempfile.TemporaryDirectory(dir=a.dir) as tmp:
        note('making the transcriptome')
        text, names, shape = transcriptome(a.records, a.names, a.seed)
        res['transcriptome'] = dict(measure('transcriptome', text, names, True, a, tmp), text=shape)
        del text
        note('making the genome shape')
        text, names, shape = genome_shape(a.contigs, a.contig_mb, a.seed)
        res['genome'] = dict(measure('genome', text, names, False, a, tmp), text=shape)
    doc = json.dumps(res, indent=1, sort_keys=True)
    print(doc)
    if a.out:
        with open(a.out, 'w') as fh:
            fh.write(doc + '\n')
    return 0


if __name__ == '__main__':
    sys.exit(main())
