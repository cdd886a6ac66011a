"""Randomised differential soak of CALL ORDER: walks of 8-14 operations drawn from the alphabet of
tests/sequence_model.py (2-D and 3-D sensor updates with changing models, parameters, scans and maps, foreign-set
scoring, both resamplers, motion, the KLD count mode, fillWeights, snapshot / restore, every init, a second filter on
the engine, statistics in both modes, the pose array, getState) at n in {257, 3000, 12000}, every operation compared
with the cache-free model, which keeps leaf / bin counts, converged, the drand48 state and the running averages itself
and takes only weights (and device-libm poses) from the engine.  A walk ends on a resample and a statistics query, so
what an earlier operation left stale is consumed.  On a mismatch one line gives the seed, the case, n, the index of the
first failing operation and the walk itself, which `--replay N "<walk>"` runs again.  No walk is skipped or retried;
the one-particle knife-edge allowance of the scoring comparisons may be used by at most 5 % of the scoring operations
of a run (counted as one more mismatch otherwise).
The row in tests/test_gpu_soaks.py runs CASES_IN_SUITE = 36 walks, 5.4 s on an MI355X against 6.7 s of the longest
other row (figures at the constant below).
usage: python tools/soak_sequences.py [cases] [seed]    |    --replay N "S2(lf,a) R(0) ..." """
import os
import sys
import time
root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, root)
sys.path.insert(0, os.path.join(root, "tests"))
import numpy as np
import badger_amcl_amd as bpf
from oracle import pyoracle as orc
import sequence_model as sm

# Chosen on an MI355X so that the row takes no longer than the longest existing row of
# test_randomised_soak_against_the_oracle.  Measured in one run of that test: soak_score-500 6.7 s (the longest),
# soak_cycle-100 6.3 s, soak_cloud-30 4.9 s; 80 walks of this tool took 13.1 s (0.16 s a walk, most of it the
# oracle's side), so 36 walks: 5.4 s measured in the same run as the 6.7 s.
CASES_IN_SUITE = 36
_world = None


def run(cases=CASES_IN_SUITE, seed=1, e=None, quiet=False):
    """Returns the number of mismatching walks (+ 1 when the knife-edge allowance was used too often)."""
    global _world
    if _world is None:
        _world = sm.World(orc)
    own = e is None
    if own:
        e = bpf.Engine(0)
    t0 = time.time()
    bad = 0
    tally = sm.Tally()
    for case, (n, ops) in enumerate(sm.soak_walks(seed, cases)):
        bad += _one(e, n, ops, tally, "seed %d case %d" % (seed, case))
        if case % 25 == 24 and not quiet:
            print("%d walks, %d mismatching, %.0f s" % (case + 1, bad, time.time() - t0), flush=True)
    share = tally.share()
    print("%d walks, %d mismatching, %d scoring operations, %d knife-edge uses (%.1f %%), %.0f s" %
          (cases, bad, tally.scoring, tally.knife, 100 * share, time.time() - t0))
    if share > 0.05:
        print("MISMATCH: the knife-edge allowance was used by more than 5 % of the scoring operations")
        bad += 1
    if own:
        e.close()
    return bad


def _one(e, n, ops, tally, label):
    d = sm.Driver(e, _world, n)
    try:
        sm.run_checked(d, sm.Model(_world, n), ops, tally)
        return 0
    except (sm.Mismatch, sm.Invalid) as m:  # (an illegal operation is the generator's fault: counted, not skipped)
        print("MISMATCH %s n %d: %s | --replay %d \"%s\"" % (label, n, m, n, sm.seq_str(ops)), flush=True)
        return 1
    finally:
        d.close()


if __name__ == "__main__":
    if len(sys.argv) > 1 and sys.argv[1] == "--replay":
        _world = sm.World(orc)
        eng = bpf.Engine(0)
        rc = _one(eng, int(sys.argv[2]), sm.parse(sys.argv[3]), sm.Tally(), "replay")
        eng.close()
        sys.exit(rc)
    sys.exit(1 if run(int(sys.argv[1]) if len(sys.argv) > 1 else 100,
                      int(sys.argv[2]) if len(sys.argv) > 2 else 1) else 0)
