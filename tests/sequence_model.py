"""A cache-free model of the filter for call-order tests: the reference's observable state -- the set, sample_count,
the leaf count with the reference's lifetime, w_slow / w_fast, converged, the 48-bit drand48 state, the resample
model and the KLD count mode -- stepped one operation at a time on top of oracle.pyoracle, plus the driver that makes
the same operation on an engine.  No GPU import at module level: tests/test_sequence_model_cpu.py steps the model
alone, tests/test_gpu_sequences.py and tools/soak_sequences.py step both and compare.

An operation is a tuple, its first element the kind:
  ("S2", cfg, scan)  PlanarScanner.updateSensor; cfg in PLANAR_CFGS (model and parameters), scan in "a" / "b"
                     (same length, other bearings, another range_max)
  ("S3",)            PointCloudScanner.updateSensor
  ("F2", how)        PlanarScanner.applyModelToSampleSet on a foreign set of another size; how = "plain" / "reg"
                     (a pageable buffer / one registered with the engine)
  ("F3",)            PointCloudScanner.applyModelToSampleSet on a foreign set of another size
  ("R", resampler)   updateResample, 0 multinomial / 1 systematic
  ("A",)             Odom.updateAction
  ("K", mode)        setKldCount, 0 leaves / 1 bins
  ("W",)             fillWeights(1 / sample_count)
  ("SN",) ("RS",)    snapshot / restore
  ("I", how)         "samples" / "half" (initWithSamples without a leaf count, the whole capacity / half of it),
                     "leaf" (initWithSamples with a leaf count), "gauss", "random"
  ("C", size)        a second ParticleFilter on the same engine: "same" / "small" / "full" capacity
  ("M",)             the other map (other cells, a LUT with another max_dist), scanner re-initialised on it
  ("Q", how)         computeClusterStats + every getClusterStats + getMaxWeightPose, "host" / "device"
  ("P",)             getPoseArray
  ("G",)             getState

What the model does NOT take from the engine: leaf count, bin count, converged, the drand48 state, w_slow, w_fast,
sample_count.  What it takes: the weights after a scoring operation (compared first, rel 1e-9, at most one knife-edge
particle, none for the beam model -- the bounds of test_gpu_parity.py / test_gpu_cloud.py) and the poses after a
motion update or a Gaussian init (compared first, 1e-12 absolute, test_gpu_motion.py's POSE_TOL: device libm), so
that everything sequential behind them -- resampling, counts, converged, the stream -- can be compared exactly."""
import ctypes as C
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)
import kld_bins_ref as kref  # noqa: E402
import pose_check_ref as pref  # noqa: E402
from scenario import Scenario, rel_err  # noqa: E402
from badger_amcl_amd import synth  # noqa: E402  (numpy only)

LEAVES, BINS = 0, 1
BEAMS = 61
ALPHA = (0.001, 0.1)          # the node's default decay rates: w_diff > 0 happens, recovery poses are drawn
MIN_SAMPLES = 100
ODOM = (2, (0.05, 0.04, 0.03, 0.02, 0.01))
ODATA = ((1.0, 2.0, 0.3), (0.03, -0.01, 0.02), (0.03, 0.01, 0.02))
GAUSS = ((5.1, 5.0, 0.3), np.eye(3), (0.4, 0.3, 0.1))
FOREIGN_N = 777               # != every filter size used
WEIGHT_RTOL = 1e-9            # test_gpu_parity.py / test_gpu_cloud.py
POSE_TOL = 1e-12              # test_gpu_motion.py
QUAT_BOUND = 2 * 1.1102230246251565e-16  # test_gpu_pose_array.py
SIZES = (257, 3000, 6000, 12000)

PLANAR_CFGS = {
    "lf": ("lf", {}),
    "lf2": ("lf", dict(sigma_hit=0.35)),
    "gompertz": ("gompertz", {}),
    "prob": ("prob", {}),
    "skip": ("prob", dict(do_beamskip=1)),
    "beam": ("beam", {}),
}
CLOUD = dict(z_hit=0.5, z_rand=0.05, sigma_hit=0.1, max_beams=128, factors=(0.95, 0.95, 0.3))
CLOUD_SHIFT = 96              # voxels: the box room of test_gpu_cloud.py moved onto the 2-D map's true pose


def op_str(op):
    return op[0] + ("(" + ",".join(str(a) for a in op[1:]) + ")" if len(op) > 1 else "")


def seq_str(ops):
    return " ".join(op_str(o) for o in ops)


def parse(text):
    """'S2(lf,a) R(0) Q(host)' -> ops; the inverse of seq_str (a failing walk is replayable from its printed line)."""
    ops = []
    for tok in text.split():
        if "(" in tok:
            kind, args = tok[:-1].split("(")
            ops.append((kind,) + tuple(int(a) if a.lstrip("-").isdigit() else a for a in args.split(",")))
        else:
            ops.append((tok,))
    return ops


# ------------------------------------------------------------------------------------------------- the shared inputs
class World:
    """Everything both sides are given: two maps, two scans, the 3-D scene and its cloud, foreign sets."""
    _cloud_cache = None

    def __init__(self, orc):
        self.orc = orc
        sc = Scenario(orc, size=200, n=64, beams=BEAMS, cloud="converged", max_dist=2.0, seed=3, frac_nan=0.0)
        self.sc = sc
        self.res, self.origin, self.pose = sc.res, sc.origin, sc.pose
        cells1 = sc.cells.copy()
        cells1[60:70, 120:140] = 1  # another obstacle: other cells, another free-space list
        self.cells = [sc.cells, cells1]
        self.max_dist = [2.0, 1.0]
        self.omaps = [sc.omap, orc.OccupancyMap(cells1, sc.res, sc.origin)]
        self.omaps[1].update_distances_lut(1.0)
        ranges_b, angles_b = synth.cast_scan(sc.cells, sc.origin, sc.res, sc.pose, BEAMS, range_max=12.0,
                                             fov=1.2 * np.pi, seed=5, frac_max=0.03)
        self.scans = {"a": (sc.ranges, sc.angles, sc.range_max), "b": (ranges_b, angles_b, 12.0)}
        self._free = {}
        # 3-D: test_gpu_cloud.py's scene, 8 x 256 rays, translated so that its true pose is the 2-D one
        if World._cloud_cache is None:
            occ = synth.box_room_voxels()
            off = CLOUD_SHIFT * 0.05
            tf_xyz, ang, yaw = (0.2, -0.1, 0.5), 0.3, 0.3
            true = np.array([0.3, 0.2])
            sx = true[0] + np.cos(yaw) * tf_xyz[0] - np.sin(yaw) * tf_xyz[1]
            sy = true[1] + np.sin(yaw) * tf_xyz[0] + np.cos(yaw) * tf_xyz[1]
            pts = synth.sphere_cloud(8, 256, (sx, sy, tf_xyz[2]), occ, 0.05, max_range=6.0, seed=4)
            a = -(yaw + ang)
            R = np.array([[np.cos(a), -np.sin(a), 0], [np.sin(a), np.cos(a), 0], [0, 0, 1]])
            pts = (pts @ R.T).astype(np.float32)
            occ = occ + np.array([CLOUD_SHIFT, CLOUD_SHIFT, 0], dtype=np.int32)
            mn, mx = occ.min(axis=0) - 3, occ.max(axis=0) + 3
            lut = orc.OctoMapLUT(mn, mx, 0.05, 0.3).build(occ)
            assert abs(true[0] + off - sc.pose[0]) < 1e-9 and abs(true[1] + off - sc.pose[1]) < 0.21
            World._cloud_cache = (lut, pts, tf_xyz, (0.0, 0.0, np.sin(ang / 2), np.cos(ang / 2)))
        self.lut3, self.pts, self.tf_xyz, self.tf_quat = World._cloud_cache
        self.cloud_p = orc.cloud(orc.CLOUD_MODEL, CLOUD["max_beams"], self.tf_xyz, self.tf_quat, z_hit=CLOUD["z_hit"],
                                 z_rand=CLOUD["z_rand"], sigma_hit=CLOUD["sigma_hit"])
        self.cloud_p.off_map_factor = CLOUD["factors"][0]
        self._samples = {}
        self.foreign = self.samples(FOREIGN_N, seed=31)

    def samples(self, n, seed=3):
        """n particles, half near the truth, half anywhere (off the map and inside walls too), uneven weights."""
        if (n, seed) not in self._samples:
            a = synth.converged_cloud(n - n // 2, self.pose, seed=seed + 10)
            b = synth.spread_cloud(n // 2, 200, self.res, seed=seed + 11)
            s = np.ascontiguousarray(np.concatenate([a, b]))
            s[:, 3] = np.random.default_rng(seed + 20).uniform(0.5, 1.5, n)
            s[:, 3] /= s[:, 3].sum()  # a set as an init leaves it: normalised (a resample may follow at once)
            self._samples[(n, seed)] = s
        return self._samples[(n, seed)].copy()

    def planar(self, cfg):
        model, kw = PLANAR_CFGS[cfg]
        return self.sc.oracle_planar(BEAMS, model, kw)

    def free_space(self, which):
        """Node2D::updateFreeSpaceIndices of map `which` for pose_check_ref's generator."""
        if which not in self._free:
            m = self.omaps[which]
            cells = pref.free_cells_2d(m.cells, m.lut, synth.MAP_FACTORS[2])
            self._free[which] = pref.FreeSpace.planar(cells, m.size_x, m.size_y, m.origin, m.resolution)
        return self._free[which]


class Invalid(Exception):
    """The operation is not legal in the model's state (the walk generator asks before it draws)."""


# ------------------------------------------------------------------------------------------------------- the model
class Model:
    def __init__(self, world, n, seed=42, alpha=ALPHA, min_samples=MIN_SAMPLES, samples=None, pop=None):
        self.w, self.orc = world, world.orc
        self.alpha, self.min_samples, self.pop = alpha, min_samples, pop
        self.kld = LEAVES
        self.map = 0
        self.snap = None
        self.zero_total = False
        self.full = n
        st = C.c_uint64(0)
        self.orc.lib().orc_srand48(C.byref(st), seed)
        self._create(n, st.value)
        self._load(world.samples(n) if samples is None else samples, None)

    # -- pieces
    def _create(self, max_samples, rng):
        opf = self.orc.ParticleFilter(min(self.min_samples, max_samples), max_samples, self.alpha[0], self.alpha[1],
                                      85.0)
        if self.pop:
            opf.set_population_size_parameters(*self.pop)
        opf.pf.rng = rng
        opf.set_random_pose_source(self.w.omaps[self.map], synth.MAP_FACTORS[2])
        self.opf = opf
        self.max = max_samples
        self.leaf, self.bins = 0, 0  # particle_filter.cpp:62-89: the constructor inserts nothing into the tree
        self.snap = None

    def _count(self, samples):
        t = self.orc.KDTree()
        for k in range(samples.shape[0]):
            t.insert_pose(samples[k, :3], samples[k, 3])
        return (t.node_count() if self.kld == BINS else t.leaf_count()), t.node_count()

    def _load(self, samples, leaf):
        self.opf.set_samples(samples, leaf_count=0)
        self.opf.pf.w_slow = self.opf.pf.w_fast = 0.0  # particle_filter.cpp:126-131,157-162
        self.opf.set_converged = self.opf.pf.converged = 0
        self.leaf, self.bins = (leaf, -1) if leaf is not None else self._count(samples)

    @property
    def n(self):
        return self.opf.sample_count

    @property
    def set(self):
        return self.opf.samples[:self.opf.sample_count]

    def state(self):
        return dict(sample_count=self.n, leaf_count=self.leaf, bin_count=self.bins, converged=self.opf.set_converged,
                    w_slow=self.opf.pf.w_slow, w_fast=self.opf.pf.w_fast, rng=int(self.opf.pf.rng))

    def adopt_weights(self, w):
        self.opf.samples[:self.n, 3] = w

    def adopt_poses(self, poses, recount=False):
        self.opf.samples[:self.n, :3] = poses
        if recount:  # the tree is built from the poses the set really has (test_init_with_gaussian_matches_oracle)
            self.leaf, self.bins = self._count(self.set)

    def adopt_averages(self, w_slow, w_fast):
        self.opf.pf.w_slow, self.opf.pf.w_fast = w_slow, w_fast

    def legal(self, op):
        k = op[0]
        if k == "RS":
            return self.snap is not None
        if k == "C":
            return True
        if k == "R":
            # particle_filter.cpp:438-440 leaves w_diff = 1 - 0 / 0 = NaN when no sensor update has run since the
            # averages were last zeroed (init, constructor, recovery reset): `NaN < 0.0` is false, and
            # resampleSystematic's `int num_random_poses = w_diff * count` (:305) is then undefined behaviour in the
            # reference.  The multinomial sampler only compares (`drand48() < NaN`: never) and stays defined.
            return not self.zero_total and (op[1] == 0 or self.opf.pf.w_slow != 0.0)
        return True

    # -- one operation; returns what the engine is expected to show for it
    def step(self, op):
        if not self.legal(op):
            raise Invalid(op_str(op))
        orc, opf, k = self.orc, self.opf, op[0]
        exp = {}
        if k == "S2":
            ranges, angles, rmax = self.w.scans[op[2]]
            p = self.w.planar(op[1])
            total = opf.update_sensor(lambda s, conv: orc.planar_apply(p, self.w.omaps[self.map], s, ranges, angles,
                                                                      rmax, conv))
            self.zero_total = not total > 0.0
            exp.update(weights=self.set[:, 3].copy(), knife=0 if op[1] == "beam" else 1)
        elif k == "S3":
            total = opf.update_sensor(lambda s, conv: orc.cloud_apply(self.w.cloud_p, self.w.lut3, s, self.w.pts))
            self.zero_total = not total > 0.0
            exp.update(weights=self.set[:, 3].copy(), knife=1)
        elif k == "F2":
            ranges, angles, rmax = self.w.scans["a"]
            f = self.w.foreign.copy()
            tot = orc.planar_apply(self.w.planar("lf"), self.w.omaps[self.map], f, ranges, angles, rmax, 0)
            exp.update(foreign=f, total=tot, knife=1)
        elif k == "F3":
            f = self.w.foreign.copy()
            tot = orc.cloud_apply(self.w.cloud_p, self.w.lut3, f, self.w.pts)
            exp.update(foreign=f, total=tot, knife=1)
        elif k == "R":
            opf.set_resample_model(op[1])
            if self.kld == LEAVES:
                out = opf.update_resample()
                assert out.status == 0
                self.leaf, self.bins = out.leaf_count, out.node_count
            else:
                self._resample_bins(op[1])
            self.zero_total = False
            exp.update(set=self.set.copy())
        elif k == "A":
            opf.pf.rng = orc.odom_update_action(ODOM[0], ODOM[1], ODATA[0], ODATA[1], ODATA[2], self.set,
                                                opf.pf.rng)
            # the tree stays the one of the poses the set was created with (abi_motion.inl, update_action)
            exp.update(poses=self.set[:, :3].copy())
        elif k == "K":
            if op[1] != self.kld:
                self.kld = op[1]
                self.leaf, self.bins = self._count(self.set)  # counted again in the new mode, from the set as it is
        elif k == "W":
            self.set[:, 3] = 1.0 / self.n
            self.zero_total = False
        elif k == "SN":
            self.snap = (self.set.copy(), self.leaf, self.bins, self.kld)
        elif k == "RS":
            s, leaf, bins, mode = self.snap
            opf.samples[:s.shape[0]] = s
            opf.sample_count = s.shape[0]
            self.leaf, self.bins = (leaf, bins) if mode == self.kld else self._count(s)
            self.zero_total = False
        elif k == "I":
            self.zero_total = False
            if op[1] in ("samples", "half", "leaf"):
                cnt = self.max if op[1] != "half" else max(self.max // 2, 1)
                self._load(self.w.samples(cnt, seed=7), 57 if op[1] == "leaf" else None)
            elif op[1] == "gauss":
                opf.init_with_gaussian(*GAUSS)
                self._after_init()
                exp.update(poses=self.set[:, :3].copy(), recount=True)
            elif op[1] == "random":
                opf.init_with_free_space_poses()
                self._after_init()
            else:
                raise ValueError(op)
            exp.update(set=self.set.copy())
        elif k == "C":
            self.full = max(self.full, self.max)
            size = dict(same=self.max, small=max(self.max // 2 + 1, 2), full=self.full)[op[1]]
            self._create(size, opf.pf.rng)  # the stream and the KLD count mode are the engine's, not the filter's
            self.zero_total = False
            exp.update(set=self.set.copy())
        elif k == "M":
            self.map ^= 1
            opf.set_random_pose_source(self.w.omaps[self.map], synth.MAP_FACTORS[2])
        elif k == "Q":
            t = orc.KDTree()
            cur = self.set
            for i in range(cur.shape[0]):
                t.insert_pose(cur[i, :3], cur[i, 3])
            exp.update(stats=t.cluster_stats(cur, cur.shape[0]))
        elif k == "P":
            exp.update(pose_array=orc.wire_pose_array(self.set))
        elif k == "G":
            exp.update(state=self.state())
        else:
            raise ValueError(op)
        return exp

    def _after_init(self):
        opf = self.opf
        opf.pf.w_slow = opf.pf.w_fast = 0.0
        opf.pf.converged = 0
        self.leaf, self.bins = (opf.node_count if self.kld == BINS else opf.leaf_count), opf.node_count

    def _resample_bins(self, resampler):
        """The BINS form has no reference run: kld_bins_ref.py is its reference (test_kld_bins_cpu.py)."""
        opf, pf = self.opf, self.opf.pf
        w_diff = 1.0 - pf.w_fast / pf.w_slow if pf.w_slow != 0.0 else 0.0
        if not w_diff >= 0.0:
            w_diff = 0.0
        r = kref.Rng(pf.rng)
        gen = pref.FastGen(self.w.free_space(self.map), 0.0, 0.0)
        want, k, leaf, nodes, _ = kref.resample(self.set.copy(), self.leaf, w_diff, r, gen, resampler, opf,
                                                self.orc.KDTree, BINS)
        M = len(want)
        opf.samples = np.zeros((self.max, 4))
        opf.samples[:M, :3] = np.array(want)
        opf.samples[:M, 3] = 1.0 / M
        opf.sample_count = M
        pf.rng = r.s
        if w_diff > 0.0:
            pf.w_slow = pf.w_fast = 0.0
        conv = self.orc.lib().orc_pf_update_converged(C.byref(pf), opf.samples.ctypes.data_as(C.POINTER(C.c_double)),
                                                      M, None)
        opf.set_converged = pf.converged = conv
        self.leaf, self.bins = k, nodes


# ------------------------------------------------------------------------------------- the engine side of every op
class Driver:
    """The same operations through badger_amcl_amd on one engine.  observe() copies the set and the drand48 state
    without touching lazily built state (bpf_pf_get_samples / bpf_pf_get_rng_state read, nothing else: getState and
    the statistics build trees and fetch scalars, which is why they are operations and not observations)."""

    def __init__(self, engine, world, n, seed=42, alpha=ALPHA, min_samples=MIN_SAMPLES, samples=None, pop=None,
                 fused=1):
        import badger_amcl_amd as bpf
        self.bpf, self.hpf = bpf, bpf.pf
        self.e, self.w = engine, world
        self.alpha, self.min_samples, self.pop = alpha, min_samples, pop
        self.map = 0
        self.full = n
        self.reg = None
        # fused = 0 (BPF_OPT_FUSED_RESAMPLE off): the sensor update's normalisation leaves tile sums for the CDF scan
        # instead of the CDF itself, and the resample takes its separate launches
        engine.set_option(self.hpf.OPT_FUSED_RESAMPLE, fused)
        engine.set_option(self.hpf.OPT_STATS_HOST, 0)
        self.stats_host = 0  # (bpf_set_option drops the statistics: switched only when a Q asks for the other mode)
        self._maps()
        self.cloud = bpf.PointCloudScanner(engine)
        om = bpf.OctoMap(engine, 0.05)
        om.setDistancesLUT(world.lut3.pose_indices, world.lut3.distance_ratios, world.lut3.min_cells,
                           world.lut3.max_cells, 0.3)
        self.cloud.init(CLOUD["max_beams"], om)
        self.cloud.setPointCloudModel(CLOUD["z_hit"], CLOUD["z_rand"], CLOUD["sigma_hit"])
        self.cloud.setMapFactors(*CLOUD["factors"])
        self.cloud.setPointCloudScannerToFootprintTF(world.tf_xyz, world.tf_quat)
        self.cdata = bpf.PointCloudData(world.pts)
        self.odom = bpf.Odom(engine)
        self.odom.setModel(ODOM[0], *ODOM[1])
        self._create(n)
        self.pf.setKldCount(LEAVES)
        self.pf.srand48(seed)
        self.pf.initWithSamples(world.samples(n) if samples is None else samples)

    def _maps(self):
        bpf, w = self.bpf, self.w
        m = bpf.OccupancyMap(self.e, w.res)
        m.setCells(w.cells[self.map])
        m.setOrigin(w.origin)
        m.setDistancesLUT(w.omaps[self.map].lut, w.max_dist[self.map])
        self.sc = bpf.PlanarScanner(self.e)
        self.sc.init(BEAMS, m)
        self.sc.setMapFactors(*synth.MAP_FACTORS)
        self.sc.setPlanarScannerPose(w.sc.scanner_pose)
        self.helper = Scenario.__new__(Scenario)
        self.helper.max_dist = w.max_dist[self.map]

    def _create(self, max_samples):
        self.pf = self.bpf.ParticleFilter(self.e, min(self.min_samples, max_samples), max_samples, self.alpha[0],
                                          self.alpha[1], 85.0)
        if self.pop:
            self.pf.setPopulationSizeParameters(*self.pop)
        self.pf.setRandomPoseGenerator(self.hpf.RANDOM_POSE_FREE_SPACE_2D)
        self.max = max_samples
        self.buf = np.empty((max_samples, 4))

    def close(self):
        self.e.set_option(self.hpf.OPT_FUSED_RESAMPLE, 1)
        self.e.set_option(self.hpf.OPT_STATS_HOST, 0)
        if self.reg is not None:
            self.e.unregisterHostBuffer(self.reg)
            self.reg = None

    def observe(self):
        n = C.c_int()
        lib, dp = self.e.lib, C.POINTER(C.c_double)
        self.e.check(lib.bpf_pf_get_samples(self.e.h, self.buf.ctypes.data_as(dp), self.max, C.byref(n)))
        return self.buf[:n.value].copy(), self.pf.getRngState()

    def step(self, op):
        bpf, pf, k = self.bpf, self.pf, op[0]
        got = {}
        if k == "S2":
            model, kw = PLANAR_CFGS[op[1]]
            self.helper.configure_gpu_model(self.sc, model, kw)
            assert self.sc.updateSensor(pf, bpf.PlanarData(*self.w.scans[op[2]]))
        elif k == "S3":
            assert self.cloud.updateSensor(pf, self.cdata)
        elif k == "F2":
            self.helper.configure_gpu_model(self.sc, "lf", {})
            if op[1] == "reg":
                if self.reg is None:
                    self.reg = np.empty((FOREIGN_N, 4))
                    self.e.registerHostBuffer(self.reg)
                f = self.reg
                f[:] = self.w.foreign
            else:
                f = self.w.foreign.copy()
            tot = self.sc.applyModelToSampleSet(bpf.PlanarData(*self.w.scans["a"]), f, 0)
            got.update(foreign=f.copy(), total=tot)
        elif k == "F3":
            f = self.w.foreign.copy()
            tot = self.cloud.applyModelToSampleSet(self.cdata, f)
            got.update(foreign=f, total=tot)
        elif k == "R":
            pf.setResampleModel(op[1])
            pf.updateResample()
        elif k == "A":
            self.odom.updateAction(pf, bpf.OdomData(*ODATA))
        elif k == "K":
            pf.setKldCount(op[1])
        elif k == "W":
            pf.fillWeights(1.0 / self._count())
        elif k == "SN":
            pf.snapshot()
        elif k == "RS":
            pf.restore()
        elif k == "I":
            if op[1] in ("samples", "half", "leaf"):
                cnt = self.max if op[1] != "half" else max(self.max // 2, 1)
                pf.initWithSamples(self.w.samples(cnt, seed=7), 57 if op[1] == "leaf" else -1)
            elif op[1] == "gauss":
                pf.initWithGaussian(*GAUSS)
            else:
                pf.initWithRandomPoses()
        elif k == "C":
            self.full = max(self.full, self.max)
            self._create(dict(same=self.max, small=max(self.max // 2 + 1, 2), full=self.full)[op[1]])
        elif k == "M":
            self.map ^= 1
            self._maps()
        elif k == "Q":
            if self.stats_host != (op[1] == "host"):
                self.stats_host = int(op[1] == "host")
                self.e.set_option(self.hpf.OPT_STATS_HOST, self.stats_host)
            n, mean, cov = pf.computeClusterStats()
            got.update(stats=dict(n=n, set_mean=mean, set_cov=cov, clusters=[pf.getClusterStats(i) for i in range(n)],
                                  past=pf.getClusterStats(n), best=pf.getMaxWeightPose()))
        elif k == "P":
            got.update(pose_array=pf.getPoseArray().copy())
        elif k == "G":
            st = pf.getState()
            got.update(state=dict(sample_count=st.sample_count, leaf_count=st.leaf_count, bin_count=st.bin_count,
                                  converged=st.converged, w_slow=st.w_slow, w_fast=st.w_fast,
                                  rng=pf.getRngState(), last_status=st.last_status))
        else:
            raise ValueError(op)
        return got

    def _count(self):
        # sample_count without getState (which would build a pending tree and fetch the scalars)
        n = C.c_int()
        self.e.check(self.e.lib.bpf_pf_get_samples(self.e.h, self.buf.ctypes.data_as(C.POINTER(C.c_double)), self.max,
                                                   C.byref(n)))
        return n.value

    def final(self):
        """Everything observable at the end of a run, for the bit-for-bit comparisons between runs."""
        s, rng = self.observe()
        st = self.step(("G",))["state"]
        q = self.step(("Q", "device"))["stats"]
        p = self.step(("P",))["pose_array"]
        return dict(set=s, rng=rng, state=st, stats=q, pose_array=p)


def same_bits(a, b):
    """Deep bit-for-bit equality of what Driver.step / Driver.final return (NaN equals NaN of the same bits)."""
    if isinstance(a, dict):
        return isinstance(b, dict) and a.keys() == b.keys() and all(same_bits(a[k], b[k]) for k in a)
    if isinstance(a, (list, tuple)):
        return isinstance(b, (list, tuple)) and len(a) == len(b) and all(same_bits(x, y) for x, y in zip(a, b))
    if isinstance(a, np.ndarray):
        return isinstance(b, np.ndarray) and a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()
    if isinstance(a, float):
        return isinstance(b, float) and np.float64(a).tobytes() == np.float64(b).tobytes()
    return a == b


# ------------------------------------------------------------------------------------------------- the comparison
class Mismatch(AssertionError):
    pass


def _need(ok, what):
    if not ok:
        raise Mismatch(what)


def _close(a, b, rtol=1e-12, atol=1e-12):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return np.allclose(a, b, rtol=rtol, atol=atol, equal_nan=True)


def _hex(a):
    return [float(v).hex() for v in np.asarray(a, dtype=np.float64).reshape(-1)]


def check_stats(got, want, exact):
    """test_gpu_next_rows.py's _assert_stats_equal on a recorded answer: the host evaluation bit for bit, the device
    evaluation within its summation-rounding budget (rel 1e-12, covariances 1e-10 absolute)."""
    n = want["n"]
    _need(got["n"] == n, "cluster count %d, oracle %d" % (got["n"], n))
    if exact:
        _need(np.array_equal(got["set_mean"], want["set_mean"]), "set mean (host, exact): %s / %s"
              % (_hex(got["set_mean"]), _hex(want["set_mean"])))
        _need(np.array_equal(got["set_cov"], want["set_cov"], equal_nan=True), "set covariance (host, exact)")
    else:
        _need(_close(got["set_mean"], want["set_mean"]), "set mean")
        _need(_close(got["set_cov"], want["set_cov"], atol=1e-10), "set covariance")
    for k in range(n):
        w, m, cnt, c = got["clusters"][k]
        _need(cnt == want["count"][k], "cluster %d count" % k)
        if exact:
            _need(w == want["weight"][k] and np.array_equal(m, want["mean"][k]) and
                  np.array_equal(c, want["cov"][k], equal_nan=True),
                  "cluster %d (host, exact): weight %r / %r, mean %s / %s, cov %s / %s"
                  % (k, w, want["weight"][k], _hex(m), _hex(want["mean"][k]), _hex(c), _hex(want["cov"][k])))
        else:
            _need(_close(w, want["weight"][k]), "cluster %d weight %r, oracle %r: statistics of other weights"
                  % (k, w, want["weight"][k]))
            _need(_close(m, want["mean"][k]) and _close(c, want["cov"][k], atol=1e-10),
                  "cluster %d (count %d, weight %r) mean %r / %r, cov %r / %r"
                  % (k, cnt, w, m, want["mean"][k], c, want["cov"][k]))
    _need(got["past"] is None, "getClusterStats past the last cluster")
    best_w, best_pose = got["best"]
    if n:
        k = int(np.argmax(want["weight"]))
        if exact:
            _need(best_w == want["weight"][k] and np.array_equal(best_pose, want["mean"][k]), "max-weight pose")
        else:
            ws = np.sort(want["weight"])[::-1]
            if ws.size < 2 or ws[0] - ws[1] > 1e-12 * ws[0]:
                _need(_close(best_w, want["weight"][k]) and _close(best_pose, want["mean"][k]),
                      "max-weight pose %r / %r, oracle %r" % (best_w, best_pose, want["weight"][k]))


class Tally:
    """Scoring operations seen and how many of them used the one-particle knife-edge allowance."""

    def __init__(self):
        self.scoring = self.knife = 0

    def share(self):
        return self.knife / self.scoring if self.scoring else 0.0


def _check_weights(got, want, allowed, tally, what):
    tally.scoring += 1
    bad = int((rel_err(got, want) > WEIGHT_RTOL).sum())
    _need(bad <= allowed, "%s: %d weights beyond rel 1e-9 (allowed %d)" % (what, bad, allowed))
    tally.knife += bad


def run_checked(driver, model, ops, tally):
    """Steps both sides; raises Mismatch(index, op, what) at the first operation whose outcome differs."""
    i, op, last_stats = -1, ("start",), None
    try:
        s, rng = driver.observe()
        _need(np.array_equal(s, model.set) and rng == int(model.opf.pf.rng), "initial set / stream")
        for i, op in enumerate(ops):
            exp = model.step(op)
            got = driver.step(op)
            s, rng = driver.observe()
            _need(s.shape[0] == model.n, "sample_count %d, model %d" % (s.shape[0], model.n))
            _need(rng == int(model.opf.pf.rng), "drand48 state %#x, model %#x" % (rng, int(model.opf.pf.rng)))
            if "weights" in exp:
                _check_weights(s[:, 3], exp["weights"], exp["knife"], tally, "weights")
                model.adopt_weights(s[:, 3])
            if "foreign" in exp:
                _check_weights(got["foreign"][:, 3], exp["foreign"][:, 3], exp["knife"], tally, "foreign weights")
                _need(np.array_equal(got["foreign"][:, :3], exp["foreign"][:, :3]), "foreign poses")
                _need(abs(got["total"] - exp["total"]) <= WEIGHT_RTOL * exp["total"], "foreign total")
            if "poses" in exp:
                d = np.abs(s[:, :3] - exp["poses"]).max()
                _need(d <= POSE_TOL, "poses off by %.3e" % d)
                model.adopt_poses(s[:, :3], exp.get("recount", False))
            elif "set" in exp:
                _need(np.array_equal(s[:, :3], exp["set"][:, :3]),
                      "poses differ from the oracle's%s" % (": a resample drawn from another CDF" if op[0] == "R"
                                                            else ""))
            if "stats" in exp:
                try:
                    check_stats(got["stats"], exp["stats"], op[1] == "host")
                except Mismatch as m:
                    if last_stats is not None and same_bits(got["stats"], last_stats[1]):
                        raise Mismatch("%s -- the answer is bit for bit the one given at op %d, before the set "
                                       "changed: stale statistics (stats_epoch not moved)" % (m, last_stats[0]))
                    raise
                last_stats = (i, got["stats"])
            if "pose_array" in exp:
                g, w_ = got["pose_array"], exp["pose_array"]
                _need(g.shape == w_.shape and np.array_equal(g[:, :5], w_[:, :5]), "pose array positions")
                _need(g.shape[0] == 0 or np.abs(g[:, 5:] - w_[:, 5:]).max() <= QUAT_BOUND, "pose array quaternions")
            if "state" in exp:
                _check_state(got["state"], exp["state"], model)
            # the whole set bit for bit: weights nobody was to touch are untouched
            _need(np.array_equal(s, model.set), "the set differs from the model's after the operation")
        exp, got = model.state(), driver.step(("G",))["state"]
        i, op = len(ops), ("G",)
        _check_state(got, exp, model)
    except Mismatch as m:
        raise Mismatch("op %d %s: %s" % (i, op_str(op), m)) from None


def _check_state(got, exp, model):
    _need(got.get("last_status", 0) == 0, "last_status %r" % got.get("last_status"))
    for key in ("sample_count", "leaf_count", "converged", "rng"):
        _need(got[key] == exp[key], "%s %r, model %r" % (key, got[key], exp[key]))
    if exp["bin_count"] >= 0:
        _need(got["bin_count"] == exp["bin_count"], "bin_count %r, model %r" % (got["bin_count"], exp["bin_count"]))
    for key in ("w_slow", "w_fast"):
        _need(abs(got[key] - exp[key]) <= WEIGHT_RTOL * abs(exp[key]), "%s %r, model %r" % (key, got[key], exp[key]))
    model.adopt_averages(got["w_slow"], got["w_fast"])


def run_blind(driver, ops):
    for op in ops:
        driver.step(op)


# ------------------------------------------------------------------------------------------ the committed sequences
def _s(text, n, **kw):
    return dict(n=n, ops=parse(text), **kw)


S2 = "S2(lf,a)"
SEQUENCES = {
    # -- the four paths of DESIGN.md section 5
    "stats_across_3d_update": _s("Q(device) S3 Q(device) Q(host) S3 Q(host)", 3000),
    # (every pose of a new filter is the origin, so WHICH CDF this resample draws from cannot show: the order is run for
    # its counts, stream and state; that the old CDF is dropped is new_set's rule, not this sequence's finding)
    "create_same_size_then_resample": _s(S2 + " C(same) R(0)", 3000),
    "create_smaller_then_stats": _s(S2 + " Q(device) C(small) Q(device) Q(host)", 3000),
    "create_after_pending_tree": _s("I(samples) C(same) G " + S2 + " R(1) G", 3000),
    "create_after_spread_init": _s("I(random) C(same) I(samples) " + S2 + " R(0)", 12000),
    # -- a foreign set must not feed the resident set's resample
    "foreign_planar_before_resample": _s(S2 + " F2(plain) R(0) " + S2 + " F2(reg) R(1)", 3000),
    "foreign_cloud_before_resample": _s(S2 + " F3 R(0) S3 F2(plain) R(1)", 3000),
    # -- statistics between updates
    "stats_between_updates": _s(S2 + " Q(device) S2(lf,b) Q(device) R(0) Q(device)", 6000),
    "stats_between_updates_host": _s(S2 + " Q(host) S2(lf,b) Q(host) R(1) Q(host)", 257),
    "motion_then_stats": _s(S2 + " R(0) A Q(device) R(1) A G Q(host)", 3000),
    "snapshot_restore": _s(S2 + " SN S2(lf,b) R(0) RS Q(device) R(0)", 3000),
    "spread_flag_across_restore": _s("I(random) " + S2 + " SN R(0) RS " + S2 + " R(0) G", 12000),
    "spread_set_resampled_whole": _s("I(random) " + S2 + " W R(0) Q(device) " + S2 + " R(0)", 12000,
                                     pop=(0.002, 3.0)),
    # -- staged-scan caches
    "sigma_changes": _s("S2(lf,a) S2(lf2,a) R(0)", 257),
    "model_changes": _s("S2(lf,a) S2(gompertz,a) S2(skip,a) S2(beam,a) R(0) S2(skip,a) S2(prob,a) R(1)", 3000),
    "scan_changes": _s("S2(lf,a) S2(lf,b) S2(lf,a) R(0)", 257),
    "map_changes": _s(S2 + " M " + S2 + " R(0) M S2(beam,a) I(random) " + S2 + " R(0)", 3000),
    # -- the KLD count mode before each consumer of the tree
    "kld_before_resample": _s(S2 + " K(1) R(1) " + S2 + " K(0) R(1) G", 3000),
    "kld_before_stats": _s(S2 + " R(0) K(1) Q(device) K(0) Q(host) G", 3000),
    "kld_before_snapshot": _s(S2 + " R(0) K(1) SN " + S2 + " R(0) K(0) RS G R(1)", 3000),
    # -- 2-D and 3-D updates of one filter
    "cloud_then_planar": _s("S3 " + S2 + " R(0) G", 6000),
    "planar_then_cloud": _s(S2 + " S3 R(1) G", 12000),
    # -- the rest of the coverage matrix
    "fill_weights": _s(S2 + " Q(device) W Q(device) R(0) " + S2 + " W R(1) Q(host) W Q(host)", 257),
    "inits": _s(S2 + " Q(device) I(gauss) Q(device) " + S2 + " R(1) I(leaf) " + S2 + " R(1) I(half) " + S2 +
                " Q(host) I(samples) Q(host) G", 3000),
    "pending_tree_into_systematic": _s("I(half) " + S2 + " R(1) G I(samples) S3 R(1) G", 3000),
    "pose_array_leaves_the_filter_alone": _s(S2 + " P R(0) P A P G", 257),
    "beam_skip_takes_converged": _s("S2(skip,a) R(0) S2(skip,a) R(0) C(same) S2(skip,a) R(1) I(samples) S2(skip,b) "
                                    "R(0) G", 3000),
}

# One sequence per row of the coverage matrix below: for every column the shortest pattern -- the row's producer, the
# column's operation, the row's consumer -- one after the other on one filter.
_COLUMN_OP = dict(S2="S2(lf,b)", S3="S3", F2="F2(plain)", F3="F3", R="R(0)", A="A", K="K(1)", W="W", RS="RS",
                  I="I(samples)", M="M", C="C(same)")
_ROWS = {  # name: (producer, consumer, n, columns left out: see EXEMPT)
    "cdf": ("S2(lf,a)", "R(0)", 6000, ()),
    "tree_and_converged": ("S2(lf,a) R(0)", "G", 3000, ("K",)),
    "converged_into_beam_skip": ("S2(lf,a) R(0)", "S2(skip,a)", 3000, ("R",)),
    "pending_tree": ("I(samples)", "G", 3000, ("A", "R")),
    "device_stats": ("Q(device)", "Q(device)", 6000, ()),
    "host_stats": ("Q(host)", "Q(host)", 257, ()),
    "spread_init": ("I(random)", "S2(lf,a)", 12000, ()),
    "scan_caches": ("S2(lf,a)", "S2(lf,a)", 257, ()),
}


def _row_sequence(producer, consumer, skip=()):
    parts = []
    for col, op in _COLUMN_OP.items():
        if col in skip:
            continue
        triple = "%s %s %s" % (producer, op, consumer)
        if col == "RS":
            triple = "SN " + triple
        if col == "K":
            triple += " K(0)"
        parts.append(triple)
    return " ".join(parts)


for _name, (_p, _c, _n, _skip) in _ROWS.items():
    SEQUENCES["matrix_" + _name] = _s(_row_sequence(_p, _c, _skip), _n)
# the cdf row again with BPF_OPT_FUSED_RESAMPLE off: the update leaves tile sums (k_normalize_fused), not the CDF
SEQUENCES["matrix_tile_sums"] = _s(_row_sequence("S2(lf,a)", "R(0)"), 6000, fused=0)

# ---------------------------------------------------------------------------------------------- the coverage matrix
COLUMNS = ("S2", "S3", "F2", "F3", "R", "A", "K", "W", "RS", "I", "C", "M")


def _is(kind, *args):
    return lambda op: op[0] == kind and (not args or op[1] in args)


def _any(*preds):
    return lambda op: any(p(op) for p in preds)


LF = ("lf", "lf2", "gompertz", "prob", "skip")
# product: (who leaves it behind, who would be served it)
PRODUCTS = {
    "cdf": (_is("S2"), _is("R")),
    "tile_sums": (_is("S2"), _is("R")),
    "tree_counts": (_any(_is("R"), _is("I", "gauss", "random"), _is("G")), _any(_is("G"), _is("R", 1), _is("SN"))),
    "pending_tree": (_any(_is("I", "samples", "half"), _is("K")), _any(_is("G"), _is("R", 1), _is("SN"), _is("A"))),
    "device_stats": (_is("Q", "device"), _is("Q", "device")),
    "host_stats": (_is("Q", "host"), _is("Q", "host")),
    "max_weight_pose": (_is("Q"), _is("Q")),
    "converged_pending": (_is("R"), _any(_is("G"), _is("S2", "skip"))),
    "spread_init": (_is("I", "random"), _is("S2", *LF)),
    "term_table": (_is("S2", *LF), _is("S2", *LF)),
    "trig_cache": (_is("S2"), _is("S2")),
}
# which committed sequences can hold a product at all: the update leaves the CDF with BPF_OPT_FUSED_RESAMPLE on (the
# default) and tile sums with it off
HOLDS = {"cdf": lambda spec: spec.get("fused", 1) == 1, "tile_sums": lambda spec: spec.get("fused", 1) == 0}
TAKEN_ONCE = ("pending_tree", "converged_pending")  # the first consumer ends them: none may sit before the column's op
_PENDING_TAKEN = ("the first consumer of a pending tree builds it: nothing pending is left for a consumer behind a %s,"
                  " which is itself that consumer or replaces the set")
EXEMPT = {}
EXEMPT.update({
    ("pending_tree", "A"): _PENDING_TAKEN % "motion update (update_action builds the tree before the poses move)",
    ("pending_tree", "R"): "a resample ends a pending tree by construction (resample_begins): its own draws are the "
                           "new set's tree; R(1) as the consumer is the pattern's third element",
    ("tree_counts", "K"): "K replaces the counts by a pending tree: the pending_tree row's producer",
    ("converged_pending", "R"): "a second resample replaces the hand-over with its own; covered as producer",
})


def coverage(sequences=None):
    """{(product, column): [(sequence name, i, j, k), ...]} over the committed sequences: producer at i, the column's
    operation at j, a consumer at k, and no operation of another non-exempt column in between."""
    sequences = SEQUENCES if sequences is None else sequences
    found = {}
    for prod, (produce, consume) in PRODUCTS.items():
        for col in COLUMNS:
            if (prod, col) in EXEMPT:
                continue
            hits = []
            for name, spec in sequences.items():
                if not HOLDS.get(prod, lambda spec: True)(spec):
                    continue
                ops = spec["ops"]
                for j, inv in enumerate(ops):
                    if inv[0] != col:
                        continue
                    # nearest producer before j and nearest consumer after j, nothing of another column between
                    i = j - 1
                    while i >= 0 and not produce(ops[i]) and not (prod in TAKEN_ONCE and consume(ops[i])) and \
                            (ops[i][0] not in COLUMNS or (prod, ops[i][0]) in EXEMPT):
                        i -= 1
                    k = j + 1
                    while k < len(ops) and not consume(ops[k]) and (ops[k][0] not in COLUMNS or
                                                                    (prod, ops[k][0]) in EXEMPT):
                        k += 1
                    if i >= 0 and produce(ops[i]) and k < len(ops) and consume(ops[k]):
                        hits.append((name, i, j, k))
            found[(prod, col)] = hits
    return found


# ----------------------------------------------------------------------------------------------------- random walks
WALK_SIZES = (257, 3000, 12000)


def soak_walks(seed, cases):
    """The (n, ops) of a soak run: tools/soak_sequences.py runs them, test_sequence_model_cpu.py checks that every
    operation of the suite's own run is legal on the model."""
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(cases):
        n = int(rng.choice(WALK_SIZES))
        out.append((n, random_walk(rng, n)))
    return out


def random_walk(rng, n):
    """8-14 operations drawn under the model's validity rules (a restore needs a snapshot of this filter; a walk ends
    on a resample and a read of the state so that whatever went stale is consumed)."""
    length = int(rng.integers(8, 15))
    kinds = ["S2"] * 5 + ["R"] * 4 + ["S3", "F2", "F3", "A", "K", "W", "SN", "RS", "I", "C", "M", "Q", "Q", "P", "G"]
    ops, have_snap, scored = [], False, False
    while len(ops) < length - 2:
        k = str(rng.choice(kinds))
        if k == "RS" and not have_snap:
            continue
        if k in ("S2", "S3"):
            scored = True
        elif k in ("I", "C", "R"):
            scored_before, scored = scored, False  # (a recovery resample zeroes the averages too: see Model.legal)
        if k == "S2":
            op = (k, str(rng.choice(list(PLANAR_CFGS))), str(rng.choice(["a", "b"])))
        elif k == "F2":
            op = (k, str(rng.choice(["plain", "reg"])))
        elif k == "R":
            op = (k, int(rng.integers(0, 2)) if scored_before else 0)
        elif k == "K":
            op = (k, int(rng.integers(0, 2)))
        elif k == "I":
            op = (k, str(rng.choice(["samples", "half", "leaf", "gauss", "random"])))
        elif k == "C":
            op = (k, str(rng.choice(["same", "small", "full"])))
            have_snap = False
        elif k == "Q":
            op = (k, str(rng.choice(["host", "device"])))
        else:
            op = (k,)
        if k == "SN":
            have_snap = True
        ops.append(op)
    ops += [("R", int(rng.integers(0, 2)) if scored else 0), ("Q", "device")]
    return ops
