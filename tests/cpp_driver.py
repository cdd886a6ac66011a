"""Compiling, feeding and running the C++ test programs of tests/cpp (a plain module: the tests/test_gpu_cpp_*.py
files import it).  The programs read a case directory through tests/cpp/shard_harness.hpp: cfg.txt of
"key value ..." lines and raw arrays as <name>.bin."""
import os
import pathlib
import socket
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def compile_driver(tmp_path, name, *flags):
    """tests/cpp/<name>.cpp against the headers and the built library; the executable in tmp_path."""
    exe = pathlib.Path(tmp_path) / name
    libdir = os.path.join(ROOT, "badger_amcl_amd")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-pthread", *flags, "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cpp", name + ".cpp"), "-o", str(exe),
                           "-L", libdir, "-lbadger_pf_hip", "-Wl,-rpath," + libdir])
    return exe


def planar_case(sc, **kw):
    """(cfg, arrays) of a scenario with the 2-D map and the likelihood-field model; kw: further cfg keys."""
    from badger_amcl_amd import synth
    cfg = dict(size=[sc.size], origin=[float(np.float32(sc.origin[0])), float(np.float32(sc.origin[1]))], res=[sc.res],
               max_dist=[sc.max_dist], max_beams=[sc.ranges.shape[0]],
               model_p=[synth.LF_DEFAULTS[k] for k in ("z_hit", "z_rand", "sigma_hit")],
               map_factors=list(sc.map_factors), scanner_pose=list(sc.scanner_pose), range_max=[sc.range_max])
    cfg.update(kw)
    arrays = dict(cells=sc.cells.astype(np.int32), lut=np.asarray(sc.lut, dtype=np.float32), samples=sc.samples,
                  ranges=sc.ranges, angles=sc.angles)
    return cfg, arrays


def write_case(d, cfg, arrays):
    """Makes the directory d with cfg.txt (None: no such file) and every array as <name>.bin; {name: path}."""
    d = pathlib.Path(d)
    d.mkdir(exist_ok=True)
    if cfg is not None:
        with open(d / "cfg.txt", "w") as f:
            for k, v in cfg.items():
                f.write(k + " " + " ".join(repr(float(x)) for x in v) + "\n")
    paths = {}
    for name, arr in arrays.items():
        paths[name] = str(d / (name + ".bin"))
        np.ascontiguousarray(arr).tofile(paths[name])
    return paths


def free_port():
    with socket.socket() as so:
        so.bind(("127.0.0.1", 0))
        return so.getsockname()[1]


def run_driver(exe, args, timeout, env=None):
    """The program with the ranks' IPC environment (or `env`); the completed process, output captured as text."""
    if env is None:
        env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0")
    return subprocess.run([str(exe)] + [str(a) for a in args], capture_output=True, text=True, env=env, timeout=timeout)


def output_lines(d, world):
    """What the forked ranks and the unsharded process printed: rank0.txt .. single.txt, in that order."""
    lines = []
    for name in ["rank%d" % r for r in range(world)] + ["single"]:
        lines += open(pathlib.Path(d) / (name + ".txt")).read().splitlines()
    return lines
