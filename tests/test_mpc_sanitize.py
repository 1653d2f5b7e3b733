"""AddressSanitizer + UndefinedBehaviorSanitizer on the host build of the sampling planner (csrc/qs_mpc.h): a stand-alone program with its own
main (tests/sanitize/drv_mpc.cpp), compiled with test_sanitizers.py's flags and run.  Nothing is loaded into Python under a sanitizer."""
import os
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
sys.path.insert(0, HERE)

from test_sanitizers import SAN  # noqa: E402


def test_mpc_host_build_is_clean_under_asan_ubsan(tmp_path):
    exe = str(tmp_path / "drv_mpc")
    subprocess.check_call(["g++", *SAN, "-std=c++17", "-Wno-unknown-pragmas", "-I" + os.path.join(REPO, "include"), "-o", exe,
                           os.path.join(HERE, "sanitize", "drv_mpc.cpp")])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    clean = r.returncode == 0 and r.stdout.startswith("ok") and "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr
    assert clean, (r.stdout[-300:], r.stderr[-2000:])
