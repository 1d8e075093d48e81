"""Build heterozygosity_from_vcf's host renderer (magot_amd/csrc/vcfhost.cpp) and
its stand-alone driver vcf_host_check.cpp host-only with AddressSanitizer +
UndefinedBehaviorSanitizer and run the driver (no GPU, nothing loaded into
Python).

    python tests/sanitize/run_vcf_host.py

Exit status: the driver's (0 = clean).
"""

import os
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
BUILD = os.path.join(HERE, 'build')
EXE = os.path.join(BUILD, 'vcf_host_check')
SOURCES = [os.path.join(ROOT, 'magot_amd', 'csrc', 'vcfhost.cpp'),
           os.path.join(HERE, 'vcf_host_check.cpp')]
FLAGS = ['-std=c++17', '-O1', '-g', '-fno-omit-frame-pointer', '--offload-arch=gfx950',
         '-x', 'hip', '--offload-host-only', '-I' + os.path.join(ROOT, 'include'),
         '-Xarch_host', '-fsanitize=address', '-Xarch_host', '-fsanitize=undefined',
         '-Xarch_host', '-fno-sanitize-recover=undefined']


def main():
    os.makedirs(BUILD, exist_ok=True)
    objs = []
    for src in SOURCES:
        obj = os.path.join(BUILD, os.path.basename(src) + '.o')
        subprocess.check_call(['/opt/rocm/bin/hipcc'] + FLAGS + ['-c', src, '-o', obj])
        objs.append(obj)
    # host link only: the sanitizer runtimes of the host compiler, none for the GPU
    link = ['/opt/rocm/bin/hipcc', '-fno-gpu-sanitize', '-fsanitize=address,undefined', '-o', EXE]
    subprocess.check_call(link + objs + ['-lpthread'])
    env = dict(os.environ, ASAN_OPTIONS='detect_leaks=1:halt_on_error=1',
               UBSAN_OPTIONS='print_stacktrace=1:halt_on_error=1')
    return subprocess.call([EXE], env=env)


if __name__ == '__main__':
    sys.exit(main())
