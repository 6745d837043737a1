"""CPU: AddressSanitizer + UBSan over the slice sampler (csrc/host_slice.hpp) driving the host backend: a stand-alone
program, nothing loaded into python and nothing near a GPU."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_slice_sampler_over_the_host_backend_under_sanitizers(tmp_path):
    csrc = os.path.join(ROOT, "turbo_amd", "csrc")
    san = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]
    # "no sanitizer runtime" is decided on a program of its own, before the code under test is compiled: every error of
    # the driver, of host_slice.hpp or of the host backend below fails the test
    probe = tmp_path / "probe.cpp"
    probe.write_text("int main() { return 0; }\n")
    probed = subprocess.run(["g++"] + san + [str(probe), "-o", str(tmp_path / "probe")], capture_output=True, text=True, timeout=300)
    if probed.returncode != 0:
        pytest.skip("this g++ has no sanitizer runtime: " + probed.stderr[-200:])
    exe = str(tmp_path / "host_slice_san")
    cmd = ["g++", "-O1", "-g", "-std=c++17"] + san + [
           "-fno-omit-frame-pointer", "-pthread", "-I" + csrc, os.path.join(ROOT, "tests", "host_slice_sanitizer_driver.cpp"),
           os.path.join(csrc, "host_backend.cpp"), "-o", exe]
    built = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    assert built.returncode == 0, built.stderr[-3000:]
    run = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert run.returncode == 0 and "ERROR" not in run.stderr and "runtime error" not in run.stderr, run.stdout + run.stderr[-3000:]
    assert run.stdout.strip().splitlines()[-1] == "ok", run.stdout
