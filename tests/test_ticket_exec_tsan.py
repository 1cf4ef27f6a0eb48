"""The executor's begin / done / complete state machine under ThreadSanitizer (no GPU): the
stand-alone harness tools/exec_ticket_harness.cpp instantiates the template of
janus_amd/csrc/prio3_exec.h over a fake policy -- 8 threads x 64 jobs with up to 8 tickets each, a
quarter of them blocking, a hold toggled from a ninth thread, both launchers, one shared eventfd.
It exits non-zero on a wrong checksum, a lost or duplicated notification, a job not done within
30 s, or (halt_on_error=1) any report of the sanitizer."""
import os
import platform
import shutil
import subprocess

from tests.conftest import ROOT


def _without_aslr():
    """The command prefix that starts a child with address-space randomisation off (a flag of that
    process alone), where this user may: GCC 11's ThreadSanitizer runtime accepts mappings only in
    fixed address windows, and a kernel with vm.mmap_rnd_bits above 28 places the program outside
    them ("unexpected memory mapping")."""
    exe = shutil.which("setarch")
    if exe:
        cmd = [exe, platform.machine(), "-R"]
        if subprocess.run(cmd + ["true"], capture_output=True).returncode == 0:
            return cmd
    return []


def test_exec_ticket_state_machine_under_tsan():
    mk = subprocess.run(["make", "-C", os.path.join(ROOT, "janus_amd"),
                         "build_asan/exec_ticket_harness"], capture_output=True, text=True)
    assert mk.returncode == 0, mk.stdout[-2000:] + mk.stderr[-2000:]
    env = dict(os.environ, TSAN_OPTIONS="halt_on_error=1")
    r = subprocess.run(_without_aslr() +
                       [os.path.join(ROOT, "janus_amd", "build_asan", "exec_ticket_harness")],
                       capture_output=True, text=True, timeout=120, env=env)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert "512 jobs (384 ticketed)" in r.stdout and "0 errors" in r.stdout, r.stdout
