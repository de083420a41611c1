"""The pure host helpers of the neighbour search (magics_amd/csrc/mgx_search.h: which kernel a search runs, rows -> CSR, the
mapping of a compacted query back to world ids, the pinned layout) on the CPU: tests/cpu_search/search_harness.cpp, a stand-alone
program built with g++ -fsanitize=address,undefined against the header alone — no HIP, nothing loaded into Python.  The harness
holds the checks (the dispatch against a table written out there); a failed check or a sanitizer report fails the run."""
import os
import subprocess

HERE = os.path.dirname(os.path.abspath(__file__))


def test_search_helpers_under_sanitizers(tmp_path):
    src = os.path.join(HERE, "cpu_search", "search_harness.cpp")
    exe = str(tmp_path / "search_harness")
    cmd = ["g++", "-std=c++17", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-o", exe, src]
    # the sanitizers' runtimes inside the program where the toolchain has them as archives: the shared AddressSanitizer runtime
    # refuses to start in a process whose environment preloads any other library
    if subprocess.run(cmd + ["-static-libasan", "-static-libubsan"], stderr=subprocess.DEVNULL).returncode != 0:
        subprocess.run(cmd, check=True)
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=120)
    out = r.stdout.decode(errors="replace")
    assert r.returncode == 0 and "search harness: 0 failed checks" in out, out[-3000:]
