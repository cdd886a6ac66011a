"""The arithmetic the two resample drivers share (badger_amcl_amd/csrc/resample_plan.hpp: the multinomial window
schedule, the systematic budget, the stream account, the target chain) with no GPU: the header has no HIP include, so
tests/cpp/resample_plan.cpp compiles it into a stand-alone program and compares it, over grids of hint x max_samples x
device_min x limit sequences and M x retries x n_random, with the drivers' earlier inline arithmetic transcribed
there.  A plain build, run as a plain executable; nothing is loaded into python."""
import os
import subprocess

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)


def test_shared_resample_arithmetic_equals_the_drivers_earlier_inline_forms(tmp_path):
    exe = tmp_path / "resample_plan"
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", "-I",
                           os.path.join(ROOT, "badger_amcl_amd", "csrc"),
                           os.path.join(ROOT, "tests", "cpp", "resample_plan.cpp"), "-o", str(exe)])
    res = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert res.returncode == 0, res.stdout + res.stderr
    assert " 0 failures" in res.stdout, res.stdout
