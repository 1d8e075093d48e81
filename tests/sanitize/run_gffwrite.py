"""Build the GFF planner (magot_amd/csrc/gffplan.cpp) and its stand-alone driver
gffwrite_check.cpp host-only with AddressSanitizer + UndefinedBehaviorSanitizer
and run the driver over the two fixtures, the NCBI fixture and the edge inputs
of tests/gffwrite_expect.py, in the three formats and both orders (no GPU,
nothing sanitized is loaded into Python).  The expected bytes come from the
object path (genome.write_gff), written to files the driver compares against;
an input the object path raises on, or whose path note is not 'native', has to
be declined.

Then the score rule as the driver restates it: ``--rule`` prints its answers for
the columns of a file, compared here with tests/gffwrite_expect.py's rule on
the declines, the edge columns and 20000 seeded ones; ``--scores`` walks every
literal of the three forms with up to 4 integer and 4 fraction digits (2.5e8)
against '%.12g' of its value, Python 2's str(float).

    python tests/sanitize/run_gffwrite.py

Exit status: 0 = clean.
"""

import os
import subprocess
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))
BUILD = os.path.join(HERE, 'build')
EXE = os.path.join(BUILD, 'gffwrite_check')
SOURCES = [os.path.join(ROOT, 'magot_amd', 'csrc', 'gffplan.cpp'),
           os.path.join(HERE, 'gffwrite_check.cpp')]
FLAGS = ['-std=c++17', '-O1', '-g', '-fno-omit-frame-pointer', '--offload-arch=gfx950',
         '-x', 'hip', '--offload-host-only', '-I' + os.path.join(ROOT, 'include'),
         '-Xarch_host', '-fsanitize=address', '-Xarch_host', '-fsanitize=undefined',
         '-Xarch_host', '-fno-sanitize-recover=undefined']
FORMAT_CODES = {'gff3': 0, 'gtf': 1, 'exon_added_gff3': 2}


def cases(tmp):
    """[(gff file, format, order, expected file or '-')]"""
    import gffwrite_expect as gx
    from magot_amd import genome
    golden = os.path.join(ROOT, 'tests', 'golden')
    inputs = [(os.path.join(golden, f), None)
              for f in ('minimalGFF3.gff', 'StandardGTF.gtf', 'O.biroi_NCBIrefseq_gff3Subset.gff')]
    for name, case in sorted(gx.cases().items()):
        path = os.path.join(tmp, name + '.gff')
        with open(path, 'wb') as fh:
            fh.write(case['gff'].encode('latin-1'))
        inputs.append((path, case))
    out = []
    for path, case in inputs:
        aset = genome.read_gff(path)
        for fmt in sorted(gx.FORMATS):
            for order in ('insertion', 'py2'):
                want = '-'
                note = 'native' if case is None else gx.path_note(case, fmt)
                if note in ('native', 'score'):
                    try:
                        text = genome.write_gff(aset, gx.FORMATS[fmt], order) + '\n'
                    except Exception:  # the reference raises: the planner declines
                        text = None
                    if text is not None and note == 'native':
                        want = '%s.%s.%s.want' % (path if case is not None else
                                                  os.path.join(tmp, os.path.basename(path)),
                                                  fmt, order)
                        with open(want, 'wb') as fh:
                            fh.write(text.encode('latin-1'))
                out.append((path, FORMAT_CODES[fmt], order, want))
    return out


def main():
    os.makedirs(BUILD, exist_ok=True)
    objs = []
    for src in SOURCES:
        obj = os.path.join(BUILD, 'gw_' + os.path.basename(src) + '.o')
        subprocess.check_call(['/opt/rocm/bin/hipcc'] + FLAGS + ['-c', src, '-o', obj])
        objs.append(obj)
    # host link only: the sanitizer runtimes of the host compiler, none for the GPU
    link = ['/opt/rocm/bin/hipcc', '-fno-gpu-sanitize', '-fsanitize=address,undefined', '-o', EXE]
    subprocess.check_call(link + objs + ['-lpthread'])
    env = dict(os.environ, ASAN_OPTIONS='detect_leaks=1:halt_on_error=1',
               UBSAN_OPTIONS='print_stacktrace=1:halt_on_error=1')
    with tempfile.TemporaryDirectory() as tmp:
        listing = os.path.join(tmp, 'cases.txt')
        with open(listing, 'w') as fh:
            for path, fmt, order, want in cases(tmp):
                fh.write('%s\t%d\t%d\t%s\n' % (path, fmt, order == 'py2', want))
        rc = subprocess.call([EXE, listing], env=env)
        rc = rc or same_rule(tmp, env)
    return rc or subprocess.call([EXE, '--scores'], env=env)


def same_rule(tmp, env):
    """the driver's score rule is the expect module's"""
    import random
    import gffwrite_expect as gx
    rnd = random.Random(20261021)
    cols = list(gx.SCORE_DECLINES) + ['.', '', '-', '+', '-.', '%', ' ', '..', '1.', '.5', '-0',
                                       '0.0000000', '000000000000000001', '0.000123456789012']
    for _ in range(20000):
        cols.append(''.join(rnd.choice('0123456789.-+e ') if rnd.random() < 0.9 else
                            rnd.choice('xN_%') for _ in range(rnd.randint(0, 16))))
    path = os.path.join(tmp, 'columns.txt')
    with open(path, 'w') as fh:
        fh.write(''.join(c + '\n' for c in cols))
    got = subprocess.run([EXE, '--rule', path], env=env, stdout=subprocess.PIPE, text=True,
                         check=True).stdout.split('\n')[:-1]
    want = [str(gx.score_text(c)) for c in cols]
    bad = [c for c, g, w in zip(cols, got, want) if g != w]
    print('gffwrite_check: %d rule column(s), %d check failure(s)' % (len(cols), len(bad)
                                                                      + (len(got) != len(want))))
    for c in bad[:5]:
        print('FAIL: rule differs on %r' % c)
    return 1 if bad or len(got) != len(want) else 0


if __name__ == '__main__':
    sys.exit(main())
