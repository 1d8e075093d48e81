"""The get_CDS_peptides lowering under AddressSanitizer + UBSan:
tests/sanitize/run_cds_lower.py builds magot_amd/csrc/gffplan.cpp and the
stand-alone driver cds_lower_check.cpp host-only and runs the driver over the
cases of tests/cdspep_expect.py in both orders (tables against the closed form,
every view read to its end) and over its diagnostic conditions (declined); any
finding aborts the driver."""
import os
import subprocess
import sys

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.mark.skipif(not os.path.exists('/opt/rocm/bin/hipcc'), reason='needs hipcc')
def test_cds_lowering_clean_under_asan_ubsan():
    res = subprocess.run([sys.executable, os.path.join(HERE, 'sanitize', 'run_cds_lower.py')],
                         stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    out = res.stdout
    assert res.returncode == 0, out[-4000:]
    assert 'cds_lower_check: 36 case(s), 0 check failure(s)' in out
    assert 'ERROR: AddressSanitizer' not in out and 'runtime error' not in out
