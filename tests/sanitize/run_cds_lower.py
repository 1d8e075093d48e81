"""Build the GFF planner (magot_amd/csrc/gffplan.cpp) and its stand-alone driver
cds_lower_check.cpp host-only with AddressSanitizer + UndefinedBehaviorSanitizer
and run the driver over the cases of tests/cdspep_expect.py in both orders and
over its diagnostic conditions, which have to decline (no GPU, nothing
sanitized is loaded into Python).  The expected tables come from the closed
form (cdspep_expect.walk), written to files the driver compares against.

    python tests/sanitize/run_cds_lower.py

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
EXE = os.path.join(BUILD, 'cds_lower_check')
SOURCES = [os.path.join(ROOT, 'magot_amd', 'csrc', 'gffplan.cpp'),
           os.path.join(HERE, 'cds_lower_check.cpp')]
FLAGS = ['-std=c++17', '-O1', '-g', '-fno-omit-frame-pointer', '--offload-arch=gfx950',
         '-x', 'hip', '--offload-host-only', '-I' + os.path.join(ROOT, 'include'),
         '-Xarch_host', '-fsanitize=address', '-Xarch_host', '-fsanitize=undefined',
         '-Xarch_host', '-fno-sanitize-recover=undefined']
NAMES_FROM = {'CDS': 0, 'transcript': 1, 'gene': 2}


def cases(tmp):
    """Listing lines for the driver."""
    import cdspep_expect as ce
    from oracle import magot_oracle as mo
    golden = os.path.join(ROOT, 'tests', 'golden')
    real = mo.get_orfs
    mo.get_orfs = lambda s, longest=False: ''  # an IndexError is no reason to decline
    lines = []
    try:
        todo = [(name,) + ce.tool_inputs(name, golden) for name in sorted(ce.TOOL_CASES)]
        fa = ce.synthetic_genome()
        for bad in sorted(ce.DIAGNOSTICS):
            kw = {'gene_length_filter': '10'} if bad == 'no_second_line' else {}
            todo.append(('bad_' + bad, fa, ce.synthetic_gff(bad=bad), kw))
        for name, fasta, gff, kw in todo:
            if kw.get('names_from', 'CDS') not in NAMES_FROM:
                continue  # the tool never lowers these
            gff_path = os.path.join(tmp, name + '.gff')
            with open(gff_path, 'wb') as fh:
                fh.write(gff.encode('latin-1'))
            contigs = os.path.join(tmp, name + '.contigs')
            with open(contigs, 'wb') as fh:
                for nm, seq in mo.read_fasta(fasta).items():
                    fh.write(('%s\t%d\n' % (nm, len(seq))).encode('latin-1'))
            for order in ('insertion', 'py2'):
                entries, exc, _ = ce.walk(fasta, gff, order=order, **kw)
                want = '-'
                if exc is None:
                    want = os.path.join(tmp, '%s.%s.want' % (name, order))
                    with open(want, 'wb') as fh:
                        fh.write(''.join('%s\t%d\t%d\n' % (nm, len(s), g)
                                         for nm, s, g in entries).encode('latin-1'))
                flt = kw.get('gene_length_filter')
                lines.append('\t'.join([gff_path, contigs, str(int(order == 'py2')),
                                        str(NAMES_FROM[kw.get('names_from', 'CDS')]),
                                        '-' if flt is None else str(int(flt)),
                                        '\x01'.join(kw.get('gene_name_filters', ())), want]))
    finally:
        mo.get_orfs = real
    return lines


def main():
    os.makedirs(BUILD, exist_ok=True)
    objs = []
    for src in SOURCES:
        obj = os.path.join(BUILD, 'cl_' + os.path.basename(src) + '.o')
        subprocess.check_call(['/opt/rocm/bin/hipcc'] + FLAGS + ['-c', src, '-o', obj])
        objs.append(obj)
    # host link only: the sanitizer runtimes of the host compiler, none for the GPU
    link = ['/opt/rocm/bin/hipcc', '-fno-gpu-sanitize', '-fsanitize=address,undefined', '-o', EXE]
    subprocess.check_call(link + objs + ['-lpthread'])
    env = dict(os.environ, ASAN_OPTIONS='detect_leaks=1:halt_on_error=1',
               UBSAN_OPTIONS='print_stacktrace=1:halt_on_error=1')
    with tempfile.TemporaryDirectory() as tmp:
        listing = os.path.join(tmp, 'cases.txt')
        with open(listing, 'wb') as fh:
            fh.write(''.join(line + '\n' for line in cases(tmp)).encode('latin-1'))
        return subprocess.call([EXE, listing], env=env)


if __name__ == '__main__':
    sys.exit(main())
