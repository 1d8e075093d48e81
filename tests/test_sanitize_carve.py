"""The ABI units' slice carve under AddressSanitizer + UBSan:
tests/sanitize/run_carve.py builds the stand-alone driver of
magot_amd/csrc/hostutil.h's Carve host-only (offsets by type and through the
fields agree, place() sets every field to base + its offset, every slice is
writable to its last element inside a buffer of exactly `used` bytes, a second
place() sets nothing) and runs it; any finding aborts the driver."""
import os
import subprocess
import sys

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.mark.skipif(not os.path.exists('/opt/rocm/bin/hipcc'), reason='needs hipcc')
def test_carve_clean_under_asan_ubsan():
    res = subprocess.run([sys.executable, os.path.join(HERE, 'sanitize', 'run_carve.py')],
                         stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    out = res.stdout
    assert res.returncode == 0, out[-4000:]
    assert 'carve_check: 0 check failure(s)' in out
    assert 'ERROR: AddressSanitizer' not in out and 'runtime error' not in out
