"""The publish-and-poll helpers of the engine's host code (badger_amcl_amd/csrc/host_poll.hpp) with no GPU: the header
has no HIP include, so a stand-alone host program compiles it, and a writer thread stands in for the kernel that
publishes a result block word by word behind a generation tag (tests/cpp/host_poll.cpp)."""
import os
import subprocess

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)


def test_engine_header_against_a_writer_thread(tmp_path):
    """A block is complete only when every word carries the generation, a block of the previous generation is refused
    with `out` untouched, a wait that never ends takes its bound (30 ms: at least that, and far less than 5 s), and the
    generation after 0x3fffffff is 1, never 0."""
    exe = tmp_path / "host_poll"
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-pthread", "-I", os.path.join(ROOT, "badger_amcl_amd", "csrc"),
                           os.path.join(ROOT, "tests", "cpp", "host_poll.cpp"), "-o", str(exe)])
    res = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert res.returncode == 0, res.stdout + res.stderr
    assert "host_poll: 0 failures" in res.stdout, res.stdout
