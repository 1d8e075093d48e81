"""The write_gff lowering under AddressSanitizer + UBSan:
tests/sanitize/run_gffwrite.py builds magot_amd/csrc/gffplan.cpp host-only with
its stand-alone driver and runs read and lower_write over the fixtures and the
edge inputs, in the three formats and both orders, against the object path's
bytes; any finding aborts the driver.  The driver then walks the score rule
over every literal of its three forms with up to 4 integer and 4 fraction
digits against Python 2's str(float), and its rule is compared with the expect
module's column by column."""
import os
import subprocess
import sys

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.mark.skipif(not os.path.exists('/opt/rocm/bin/hipcc'), reason='needs hipcc')
def test_gffwrite_lowering_clean_under_asan_ubsan():
    res = subprocess.run([sys.executable, os.path.join(HERE, 'sanitize', 'run_gffwrite.py')],
                         stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    out = res.stdout
    assert res.returncode == 0, out[-4000:]
    assert 'case(s), 0 check failure(s)' in out
    # the whole product of the score rule's three forms, up to 4 + 4 digits, both signs:
    # 2 * (11110 + 11111 * 11111 - 1) literals against '%.12g'
    assert 'gffwrite_check: %d score literal(s), 0 check failure(s)' % \
        (2 * (11110 + 11111 * 11111 - 1)) in out
    assert 'gffwrite_check: 20036 rule column(s), 0 check failure(s)' in out
    assert 'gffwrite_check: 0 case(s)' not in out
    assert 'ERROR: AddressSanitizer' not in out and 'runtime error' not in out
