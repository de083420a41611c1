"""The rule by which mgx_iterate merges back-to-back schedules into one post while the lingering launch is behind
(post_merge_decide / linger_plan_fits, magics_amd/csrc/mgx_resident.h) on the CPU: tests/cpu_resident/post_merge_harness.cpp, a
stand-alone program built with g++ -fsanitize=address,undefined against the header alone — no HIP, nothing loaded into Python.
The harness holds the cases (previous post taken / untaken; 10 + 10 + 10 segments fit, a fourth does not; a 32-segment schedule
alone; more than 32 segments never recorded; a schedule that opens with an external iteration; launch ended meanwhile); a failed
check or a sanitizer report fails the run."""
import os
import subprocess

HERE = os.path.dirname(os.path.abspath(__file__))


def test_post_merge_decisions_under_sanitizers(tmp_path):
    src = os.path.join(HERE, "cpu_resident", "post_merge_harness.cpp")
    exe = str(tmp_path / "post_merge_harness")
    cmd = ["g++", "-std=c++17", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-o", exe, src]
    # the sanitizers' runtimes inside the program where the toolchain has them as archives: the shared AddressSanitizer runtime
    # refuses to start in a process whose environment preloads any other library
    if subprocess.run(cmd + ["-static-libasan", "-static-libubsan"], stderr=subprocess.DEVNULL).returncode != 0:
        subprocess.run(cmd, check=True)
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=120)
    out = r.stdout.decode(errors="replace")
    assert r.returncode == 0 and "post merge harness: 0 failed checks" in out, out[-3000:]
