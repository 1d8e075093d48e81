"""heterozygosity_from_vcf's host renderer under AddressSanitizer + UBSan:
tests/sanitize/run_vcf_host.py builds magot_amd/csrc/vcfhost.cpp host-only with
its stand-alone driver (fixed counts with known text, loci of no length left
out, seeded counts on several thread counts against a restated model, bad
arguments refused) and runs it; any finding aborts the driver."""
import os
import subprocess
import sys

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.mark.skipif(not os.path.exists('/opt/rocm/bin/hipcc'), reason='needs hipcc')
def test_vcf_host_renderer_clean_under_asan_ubsan():
    res = subprocess.run([sys.executable, os.path.join(HERE, 'sanitize', 'run_vcf_host.py')],
                         stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    out = res.stdout
    assert res.returncode == 0, out[-4000:]
    assert 'vcf_host_check: 0 check failure(s)' in out
    assert 'ERROR: AddressSanitizer' not in out and 'runtime error' not in out
