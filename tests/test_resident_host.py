"""The host arithmetic of resident and lingering schedule launches (magics_amd/csrc/mgx_resident.h: a schedule's plan bytes cut
into launches, parity and segment count through launches, posts and a take-back, the back-off after declined launches) on the
CPU: tests/cpu_resident/resident_harness.cpp, a stand-alone program built with g++ -fsanitize=address,undefined against the
header alone — no HIP, nothing loaded into Python.  The harness holds the checks (against values written out there by hand); a
failed check or a sanitizer report fails the run."""
import os
import subprocess

HERE = os.path.dirname(os.path.abspath(__file__))


def test_resident_helpers_under_sanitizers(tmp_path):
    src = os.path.join(HERE, "cpu_resident", "resident_harness.cpp")
    exe = str(tmp_path / "resident_harness")
    cmd = ["g++", "-std=c++17", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-o", exe, src]
    # the sanitizers' runtimes inside the program where the toolchain has them as archives: the shared AddressSanitizer runtime
    # refuses to start in a process whose environment preloads any other library
    if subprocess.run(cmd + ["-static-libasan", "-static-libubsan"], stderr=subprocess.DEVNULL).returncode != 0:
        subprocess.run(cmd, check=True)
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=120)
    out = r.stdout.decode(errors="replace")
    assert r.returncode == 0 and "resident harness: 0 failed checks" in out, out[-3000:]
