"""besthits_from_psl's host functions under AddressSanitizer + UBSan:
tests/sanitize/run_psl_host.py builds magot_amd/csrc/pslhost.cpp host-only
with its stand-alone driver (the dict order on fixed and seeded hash arrays with
repeated low bits against a restated model, the renderer into exact-size
buffers) and runs it; any finding aborts the driver."""
import os
import subprocess
import sys

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.mark.skipif(not os.path.exists('/opt/rocm/bin/hipcc'), reason='needs hipcc')
def test_psl_host_functions_clean_under_asan_ubsan():
    res = subprocess.run([sys.executable, os.path.join(HERE, 'sanitize', 'run_psl_host.py')],
                         stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    out = res.stdout
    assert res.returncode == 0, out[-4000:]
    assert 'psl_host_check: 0 check failure(s)' in out
    assert 'ERROR: AddressSanitizer' not in out and 'runtime error' not in out
