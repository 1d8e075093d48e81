"""composition_by_site's host renderer under AddressSanitizer + UBSan:
tests/sanitize/run_site_host.py builds magot_amd/csrc/sitehost.cpp host-only
with its stand-alone driver (fixed counts with known text, seeded counts on
several thread counts against a restated model, empty sites reported with
nothing allocated) and runs it; any finding aborts the driver."""
import os
import subprocess
import sys

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.mark.skipif(not os.path.exists('/opt/rocm/bin/hipcc'), reason='needs hipcc')
def test_site_host_renderer_clean_under_asan_ubsan():
    res = subprocess.run([sys.executable, os.path.join(HERE, 'sanitize', 'run_site_host.py')],
                         stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    out = res.stdout
    assert res.returncode == 0, out[-4000:]
    assert 'site_host_check: 0 check failure(s)' in out
    assert 'ERROR: AddressSanitizer' not in out and 'runtime error' not in out
