"""The purge_overlaps planner under AddressSanitizer + UBSan:
tests/sanitize/run_overlap_plan.py builds magot_amd/csrc/overlapplan.cpp
host-only with its stand-alone driver (fixed cases, every prefix of a valid GFF
as either file, seeded mutations, the output pass into exact-size buffers) and
runs it; any finding aborts the driver."""
import os
import subprocess
import sys

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.mark.skipif(not os.path.exists('/opt/rocm/bin/hipcc'), reason='needs hipcc')
def test_overlap_planner_clean_under_asan_ubsan():
    res = subprocess.run([sys.executable, os.path.join(HERE, 'sanitize', 'run_overlap_plan.py')],
                         stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    out = res.stdout
    assert res.returncode == 0, out[-4000:]
    assert 'overlap_plan_check: 0 check failure(s)' in out
    assert 'ERROR: AddressSanitizer' not in out and 'runtime error' not in out
