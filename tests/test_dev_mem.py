"""turbo_amd/csrc/dev_mem.hpp on the CPU: the owners of a handle's device memory, pinned memory and events, instantiated
over a counting malloc policy (tests/dev_mem_sanitizer_driver.cpp) -- no HIP header, nothing loaded into python, no GPU."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_owners_under_sanitizers(tmp_path):
    """AddressSanitizer + UBSan + the leak check over reserve()'s contract (no-op, grow, failing synchronisation, failing
    allocation, failing view), move-assignment of a group, destruction of full and empty owners"""
    san = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]
    # "no sanitizer runtime" is decided on a program of its own, before the code under test is compiled: every error of
    # the driver or the header below fails the test
    probe = tmp_path / "probe.cpp"
    probe.write_text("int main() { return 0; }\n")
    probed = subprocess.run(["g++"] + san + [str(probe), "-o", str(tmp_path / "probe")], capture_output=True, text=True, timeout=300)
    if probed.returncode != 0:
        pytest.skip("this g++ has no sanitizer runtime: " + probed.stderr[-200:])
    exe = str(tmp_path / "dev_mem_san")
    cmd = ["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Werror"] + san + [
           "-fno-omit-frame-pointer", "-I" + os.path.join(ROOT, "turbo_amd", "csrc"),
           os.path.join(ROOT, "tests", "dev_mem_sanitizer_driver.cpp"), "-o", exe]
    built = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    assert built.returncode == 0, built.stderr[-3000:]
    run = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert run.returncode == 0 and "ERROR" not in run.stderr and "runtime error" not in run.stderr, run.stdout[-1000:] + run.stderr[-3000:]
    assert run.stdout.startswith("dev_mem ok: "), run.stdout
