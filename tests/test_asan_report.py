"""The host form of the DAP `Report` decoder (the leader's upload handler reads untrusted bytes)
built with AddressSanitizer and driven by tools/fuzz_report.cpp over mutated Report rows (bit
flips, truncations, length-field extremes, splices, report_len above the row), each in an
allocation that ends where the readable bytes end.  A stand-alone program: CPU only, nothing is
loaded into Python; any heap over-read / over-write aborts the harness with an ASan report."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.skipif(shutil.which("/opt/rocm/bin/hipcc") is None, reason="hipcc not present")
def test_report_host_decoder_under_asan():
    mk = subprocess.run(["make", "-C", os.path.join(ROOT, "janus_amd"), "build_asan/fuzz_report"],
                        capture_output=True, text=True, timeout=600)
    assert mk.returncode == 0, mk.stdout + mk.stderr
    r = subprocess.run([os.path.join(ROOT, "janus_amd", "build_asan", "fuzz_report"), "20000", "7"],
                       capture_output=True, text=True, timeout=300,
                       env=dict(os.environ, ASAN_OPTIONS="detect_leaks=0:abort_on_error=1"))
    assert r.returncode == 0 and "no ASan report" in r.stdout, r.stdout + r.stderr
