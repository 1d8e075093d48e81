"""What fqstats must print (genome_tools.py:85-124), restated over a list of
lengths, a seeded FASTQ generator, and the loader of the reference's own
recorded results (tests/golden/fqstats.json, written by
golden/make_golden_fqstats.py).  Not a test module: test_fqstats_host.py and
test_gpu_fqstats.py import it, and so does the golden generator, for the one
generator both sides use."""

import json
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, 'golden')
KEYS = ('reads', 'bases', 'median', 'reads25', 'reads75', 'n25', 'n50', 'n75')


def load():
    with open(os.path.join(GOLDEN, 'fqstats.json')) as fh:
        return json.load(fh)


def read_lengths(data):
    """The recorded length of every sequence line of FASTQ bytes: lines end at
    LF only, line k (from 0) counts when k % 4 == 1, and its length is the line
    with its LF minus one -- so a last line without LF counts one short."""
    lines = data.split(b'\n')
    ended = lines[:-1]  # each of these had an LF
    out = [len(ln) for k, ln in enumerate(ended) if k % 4 == 1]
    if lines[-1] and len(ended) % 4 == 1:
        out.append(len(lines[-1]) - 1)
    return out


def figures(lengths):
    """The tool's figures from the lengths, every division floored (Python 2
    integers); an N-value that is never set stays None.  No reads:
    ZeroDivisionError."""
    desc = sorted(lengths, reverse=True)
    n, bp = len(desc), sum(desc)
    mean = bp // n
    out = {'reads': n, 'bases': bp, 'mean': mean, 'median': desc[n // 2], 'reads25': desc[n // 4],
           'reads75': desc[n * 3 // 4], 'n25': None, 'n50': None, 'n75': None}
    running = 0
    for length in desc:
        running += length
        for key, mark in (('n25', bp // 4), ('n50', bp // 2), ('n75', bp * 3 // 4)):
            if out[key] is None and running > mark:
                out[key] = length
    return out


def text_of(f):
    """The nine lines"""
    show = lambda v: 'False' if v is None else str(v)  # noqa: E731
    return ('%d reads\ntotal basepairs=%d\nmedian length=%d\nmean length=%d\n'
            '25%% of reads >%d\n75%% of reads >%d\n' % (f['reads'], f['bases'], f['median'],
                                                        f['mean'], f['reads25'], f['reads75']) +
            'n25=%s\nn50=%s\nn75=%s\n' % (show(f['n25']), show(f['n50']), show(f['n75'])))


def expected(data):
    """(stdout text, exception name) for FASTQ bytes"""
    try:
        return text_of(figures(read_lengths(data))), None
    except ZeroDivisionError:
        return '', 'ZeroDivisionError'


def figures_from_histogram(lengths, counts):
    """figures() of the multiset (lengths ascending, counts)"""
    return figures(np.repeat(np.asarray(lengths), np.asarray(counts)).tolist())


def record(name, length, rng=None, eol=b'\n'):
    """One four-line record with a sequence line of ``length`` bytes"""
    if rng is None:
        seq = b'A' * length
    else:
        seq = np.frombuffer(b'ACGT', np.uint8)[rng.integers(0, 4, length)].tobytes()
    return b'@' + name + eol + seq + eol + b'+' + eol + b'I' * length + eol


def random_fastq(rng, n_reads=None, eol=b'\n'):
    """A small seeded FASTQ: reads of 0..40 bytes, now and then a stray line
    at the end so that the line count takes every residue mod 4, now and then
    no final LF."""
    n = int(rng.integers(0, 12)) if n_reads is None else n_reads
    text = b''.join(record(b'r%d' % k, int(rng.integers(0, 41)), rng, eol) for k in range(n))
    extra = int(rng.integers(0, 4))
    text += b''.join([b'@last' + eol, b'ACGTTGCA' * int(rng.integers(0, 3)) + eol,
                      b'+' + eol][:extra])
    if text and rng.random() < 0.3:
        text = text[:-1]
    return text
