"""Build the stand-alone driver carve_check.cpp of the ABI units' slice carve
(magot_amd/csrc/hostutil.h: Carve) host-only with AddressSanitizer +
UndefinedBehaviorSanitizer and run it (no GPU, nothing loaded into Python).

    python tests/sanitize/run_carve.py

Exit status: the driver's (0 = clean).
"""

import os
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
BUILD = os.path.join(HERE, 'build')
EXE = os.path.join(BUILD, 'carve_check')
SOURCE = os.path.join(HERE, 'carve_check.cpp')
FLAGS = ['-std=c++17', '-O1', '-g', '-fno-omit-frame-pointer', '-Wall', '--offload-arch=gfx950',
         '-x', 'hip', '--offload-host-only', '-I' + os.path.join(ROOT, 'include'),
         '-Xarch_host', '-fsanitize=address', '-Xarch_host', '-fsanitize=undefined',
         '-Xarch_host', '-fno-sanitize-recover=undefined']


def main():
    os.makedirs(BUILD, exist_ok=True)
    obj = os.path.join(BUILD, 'carve_check.cpp.o')
    subprocess.check_call(['/opt/rocm/bin/hipcc'] + FLAGS + ['-c', SOURCE, '-o', obj])
    # host link only: the sanitizer runtimes of the host compiler, none for the GPU
    subprocess.check_call(['/opt/rocm/bin/hipcc', '-fno-gpu-sanitize',
                           '-fsanitize=address,undefined', '-o', EXE, obj, '-lpthread'])
    env = dict(os.environ, ASAN_OPTIONS='detect_leaks=1:halt_on_error=1',
               UBSAN_OPTIONS='print_stacktrace=1:halt_on_error=1')
    return subprocess.call([EXE], env=env)


if __name__ == '__main__':
    sys.exit(main())
