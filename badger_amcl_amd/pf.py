"""Host-side mirror of the reference interface for the hot path, on top of the C-ABI.

Class and method names follow the reference (include/amcl/...): OccupancyMap,
PlanarData, PlanarScanner, ParticleFilter -- so a parity test reads like the reference's
own call sequence:

    map = OccupancyMap(engine, resolution); map.setSize(...); map.setOrigin(...); ...
    scanner = PlanarScanner(engine); scanner.init(max_beams, map)
    scanner.setModelLikelihoodField(z_hit, z_rand, sigma_hit, max_dist)
    pf = ParticleFilter(engine, min_samples, max_samples, alpha_slow, alpha_fast, thr)
    scanner.updateSensor(pf, data); pf.updateResample()

All computation happens in libbadger_pf_hip.so on the GPU.  This module only marshals.
"""
import ctypes as C
import math

import numpy as np

from . import _lib

MODEL_BEAM, MODEL_LIKELIHOOD_FIELD, MODEL_LIKELIHOOD_FIELD_PROB, MODEL_LIKELIHOOD_FIELD_GOMPERTZ = 0, 1, 2, 3
PF_RESAMPLE_MULTINOMIAL, PF_RESAMPLE_SYSTEMATIC = 0, 1
RANDOM_POSE_NONE, RANDOM_POSE_FREE_SPACE_2D, RANDOM_POSE_FREE_SPACE_3D = 0, 1, 2
POSE_CHECK_AS_REFERENCE, POSE_CHECK_SENSOR_MODEL = 0, 1
# what the KLD stop rule counts (bpf_pf_set_kld_count): the reference's tree leaves (default), or the distinct
# histogram bins of KLD-sampling and upstream AMCL (opt-in, parity unpinned by construction)
KLD_COUNT_LEAVES, KLD_COUNT_BINS = 0, 1
OPT_CDF_SERIAL, OPT_COUNT_CELLS, OPT_WINDOW_PATH, OPT_KLD_DEVICE_MIN, OPT_GRADED_SHARES = 0, 1, 2, 3, 4
OPT_FUSED_RESAMPLE = 5
OPT_CLOUD_DENSE = 6
OPT_STATS_HOST = 7
OPT_LUT_HOST = 8
OPT_KLD_PERSISTENT = 9
OPT_LUT_EXACT_EDT = 10
OPT_HOST_AUTO_REGISTER = 11
OPT_SEAM_CHUNKS = 12
OPT_KLD_LOCAL = 13
OPT_TILE_SORT = 14
OPT_HOST_DIRECT_PAGEABLE = 15  # pageable buffers straight to the HIP runtime (the caller promises they never move)
OPT_FUSED_LDS_TREE = 16  # the LDS form of the single-block resample's histogram tree (tests)
OPT_STAGE_ON_HOST = 17  # the host forms the scan's end points always (A/B switch of the device staging)
CELL_FREE, CELL_UNKNOWN, CELL_OCCUPIED = -1, 0, 1
# pruned pose search: the block sizes it takes and the default (profiles/pose_search_pruned.md)
POSE_SEARCH_BLOCKS = _lib.POSE_SEARCH_BLOCKS
POSE_SEARCH_BLOCK = 8
POSE_SEARCH_CLOUD_BLOCK = 16  # the cloud scanner's default (profiles/pose_search_cloud_pruned.md)
POSE_SEARCH_STATS_FIELDS = tuple(name for name, _ in _lib.PoseSearchStats._fields_)


class BpfError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__("bpf error %d: %s" % (code, msg))
        self.code = code


def _dp(a):
    return a.ctypes.data_as(C.POINTER(C.c_double))


class Engine:
    """One HIP engine = one GPU-resident map + scanner model + particle filter."""

    def __init__(self, device=0):
        self.lib = _lib.load()
        h = C.c_void_p()
        rc = self.lib.bpf_create(device, C.byref(h))
        if rc != 0:
            raise BpfError(rc, "bpf_create failed (%s)" % self.lib.bpf_error_string(rc).decode())
        self.h = h
        self.device = device

    def close(self):
        if getattr(self, "h", None):
            self.lib.bpf_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def check(self, rc):
        if rc != 0:
            raise BpfError(rc, self.lib.bpf_last_error_message(self.h).decode() or
                           self.lib.bpf_error_string(rc).decode())

    def set_stream(self, hip_stream):
        """hip_stream: a hipStream_t handle as an int (0 = HIP's default stream), or None for the
        engine's own stream."""
        handle = C.c_void_p(-1) if hip_stream is None else C.c_void_p(hip_stream)
        self.check(self.lib.bpf_set_stream(self.h, handle))

    def synchronize(self):
        self.check(self.lib.bpf_synchronize(self.h))

    def profile_enable(self, on=1):
        """1 = time every 8th launch of the scoring kernel, 3 = every launch of it, 2 = every kernel class, 0 = off."""
        self.check(self.lib.bpf_profile_enable(self.h, int(on)))

    def profile_reset(self):
        self.check(self.lib.bpf_profile_reset(self.h))

    def profile_get(self):
        p = _lib.Profile()
        self.check(self.lib.bpf_profile_get(self.h, C.byref(p)))
        names = ["score", "reduce", "normalize", "cdf", "draw", "finalize", "score_window", "score_aux", "motion"]
        return {n: {"ms": p.ms[i], "launches": p.launches[i]} for i, n in enumerate(names)}

    def registerHostBuffer(self, array):
        """Pins a caller-owned numpy buffer for the host-buffer entry points (bpf_host_buffer_register): the owner
        keeps it allocated until unregisterHostBuffer / close."""
        self.check(self.lib.bpf_host_buffer_register(self.h, C.c_void_p(array.ctypes.data), array.nbytes))

    def unregisterHostBuffer(self, array):
        self.check(self.lib.bpf_host_buffer_unregister(self.h, C.c_void_p(array.ctypes.data)))

    def isHostBufferRegistered(self, array):
        return bool(self.lib.bpf_host_buffer_is_registered(self.h, C.c_void_p(array.ctypes.data), array.nbytes))

    def score_last_form(self):
        """3 = the last scoring launch of a resident set walked the particles in map-tile order, 0 = index order."""
        a = C.c_int()
        self.check(self.lib.bpf_score_last_form(self.h, C.byref(a)))
        return a.value

    def kld_last_form(self):
        """2 = the last device-side histogram tree was grown in LDS-sized pieces, 1 = level loop, 3 = persistent."""
        a = C.c_int()
        self.check(self.lib.bpf_kld_last_form(self.h, C.byref(a)))
        return a.value

    def cloud_last_form(self):
        """0 = no point-cloud launch yet, otherwise 32 | bits of the k_cloud_score instance the last one took:
        1 = exact reciprocal, 2 = PLANAR, 4 = DENSE, 8 = BORDER, 16 = graded partition on."""
        a = C.c_int()
        self.check(self.lib.bpf_cloud_last_form(self.h, C.byref(a)))
        return a.value

    def seam_last_plan(self):
        """(chunks, pinned) of the last applyModelToSampleSet: 0 chunks = the plain upload / score / download, -1 = one
        launch that read and wrote the registered records in place."""
        a, b = C.c_int(), C.c_int()
        self.check(self.lib.bpf_seam_last_plan(self.h, C.byref(a), C.byref(b)))
        return a.value, bool(b.value)

    def set_option(self, option, value):
        self.check(self.lib.bpf_set_option(self.h, option, int(value)))

    def cells_walked(self, reset=True):
        v = C.c_ulonglong()
        self.check(self.lib.bpf_get_cells_walked(self.h, C.byref(v), int(reset)))
        return v.value

    def window_plan(self):
        a, b, c = C.c_int(), C.c_int(), C.c_int()
        self.check(self.lib.bpf_get_window_plan(self.h, C.byref(a), C.byref(b), C.byref(c)))
        return dict(used_window=bool(a.value), chunks_covered=b.value, chunks_total=c.value)

    def score_kernel_name(self):
        return self.lib.bpf_score_kernel_name(self.h).decode()


class OccupancyMap:
    """include/amcl/map/occupancy_map.h:54-123 (state only; queries run on the GPU)."""

    def __init__(self, engine, resolution):
        self.e = engine
        self.resolution = float(resolution)
        self.size_x = self.size_y = 0
        self.origin = (np.float32(0), np.float32(0))
        self.cells = None
        self.max_distance_to_object = 0.0
        self.lut = None
        self._dirty = True

    def setSize(self, size_vec):
        self.size_x, self.size_y = int(size_vec[0]), int(size_vec[1])
        self.cells = np.zeros((self.size_y, self.size_x), dtype=np.int32)
        self._dirty = True

    def getSize(self):
        return [self.size_x, self.size_y]

    def setOrigin(self, origin_xy):
        self.origin = (np.float32(origin_xy[0]), np.float32(origin_xy[1]))  # pcl::PointXYZ is float
        self._dirty = True

    def computeCellIndex(self, i, j):
        return i + j * self.size_x

    def setCellState(self, index, state):
        self.cells.reshape(-1)[index] = state
        self._dirty = True

    def setCells(self, cells):
        cells = np.ascontiguousarray(cells, dtype=np.int32)
        self.size_y, self.size_x = cells.shape
        self.cells = cells
        self._dirty = True

    def setDistancesLUT(self, lut, max_distance_to_object):
        """Adopt a host-built distances_lut_ (e.g. the reference's brushfire output)."""
        self.lut = np.ascontiguousarray(lut, dtype=np.float32)
        self.max_distance_to_object = float(max_distance_to_object)
        self._dirty = True

    def upload(self):
        if not self._dirty:
            return
        lutp = self.lut.ctypes.data_as(C.POINTER(C.c_float)) if self.lut is not None else None
        self.e.check(self.e.lib.bpf_map2d_set(self.e.h, self.cells.ctypes.data_as(C.POINTER(C.c_int32)), lutp,
                                              self.size_x, self.size_y, float(self.origin[0]), float(self.origin[1]),
                                              self.resolution, self.max_distance_to_object))
        self._dirty = False

    def updateDistancesLUT(self, max_distance_to_object):
        """OccupancyMap::updateDistancesLUT (occupancy_map.cpp:138-252): the reference's priority-queue brushfire, its
        values bit for bit (host builder, once per map as in the reference)."""
        self.upload()
        self.e.check(self.e.lib.bpf_map2d_build_distances_lut_reference(self.e.h, float(max_distance_to_object)))
        self.max_distance_to_object = float(max_distance_to_object)
        self.lut = None

    updateDistancesLUTReference = updateDistancesLUT

    def updateDistancesLUTExact(self, max_distance_to_object):
        """NOT a reference method: the exact capped EDT built on the device (milliseconds); <= the brushfire's values
        and different from them in < 1 % of the cells -- the caller's explicit choice."""
        self.upload()
        self.e.check(self.e.lib.bpf_map2d_build_distances_lut(self.e.h, float(max_distance_to_object)))
        self.max_distance_to_object = float(max_distance_to_object)
        self.lut = None

    def calcRange(self, ox, oy, oa, max_range):
        """OccupancyMap::calcRange (occupancy_map.cpp:257-364), batched: arrays of origins, angles and max ranges."""
        self.upload()  # the cells alone are enough (no distance LUT needed), as for the reference's calcRange
        ox, oy, oa = (np.ascontiguousarray(np.atleast_1d(v), dtype=np.float64) for v in (ox, oy, oa))
        mr = np.ascontiguousarray(np.broadcast_to(np.asarray(max_range, dtype=np.float64), ox.shape))
        # libm's cos / sin (what the reference calls), not numpy's vector loops, which may differ in the last bit
        ca = np.array([math.cos(a) for a in oa], dtype=np.float64)
        sa = np.array([math.sin(a) for a in oa], dtype=np.float64)
        out = np.zeros(ox.shape[0], dtype=np.float64)
        self.e.check(self.e.lib.bpf_map2d_calc_range(self.e.h, _dp(ox), _dp(oy), _dp(ca), _dp(sa), _dp(mr),
                                                     ox.shape[0], _dp(out)))
        return out

    def getDistancesLUT(self):
        out = np.zeros((self.size_y, self.size_x), dtype=np.float32)
        self.e.check(self.e.lib.bpf_map2d_get_distances_lut(self.e.h, out.ctypes.data_as(C.POINTER(C.c_float)),
                                                            out.size))
        return out


class PlanarData:
    """include/amcl/sensors/planar_scanner.h:45-54"""

    def __init__(self, ranges, angles, range_max):
        self.ranges_ = np.ascontiguousarray(ranges, dtype=np.float64)
        self.angles_ = np.ascontiguousarray(angles, dtype=np.float64)
        self.range_count_ = int(self.ranges_.shape[0])
        self.range_max_ = float(range_max)
        self._ptr_of = None

    def pointers(self):
        """(ranges, angles) as C pointers; formed once per pair of arrays (numpy's ctypes view costs ~2 us a time)."""
        if self._ptr_of is None or self._ptr_of[0] is not self.ranges_ or self._ptr_of[1] is not self.angles_:
            self._ptr_of = (self.ranges_, self.angles_, _dp(self.ranges_), _dp(self.angles_))
        return self._ptr_of[2], self._ptr_of[3]


class PFSampleSet:
    """View of the current sample set copied to the host (particle_filter.h:70-87)."""

    def __init__(self, samples, state):
        self.samples = samples  # [N,4] x, y, theta, weight
        self.sample_count = state.sample_count
        self.converged = state.converged
        self.leaf_count = state.leaf_count


class ParticleFilter:
    """include/amcl/pf/particle_filter.h:92-184 on the GPU-resident set."""

    def __init__(self, engine, min_samples, max_samples, alpha_slow, alpha_fast,
                 global_localization_convergence_threshold, random_pose_fn=None):
        self.e = engine
        self.max_samples = max_samples
        self.min_samples = min_samples
        self.random_pose_fn = random_pose_fn
        engine.check(engine.lib.bpf_pf_create(engine.h, min_samples, max_samples, alpha_slow, alpha_fast,
                                              global_localization_convergence_threshold))

    resample_model = PF_RESAMPLE_MULTINOMIAL

    def setResampleModel(self, model):
        self.resample_model = int(model)
        self._setResampleModel(model)

    def _setResampleModel(self, model):
        self.e.check(self.e.lib.bpf_pf_set_resample_model(self.e.h, model))

    def setRandomPoseGenerator(self, mode):
        """random_pose_fn of the reference's constructor: RANDOM_POSE_FREE_SPACE_2D = Node::randomFreeSpacePose over
        Node2D's free-space list, RANDOM_POSE_FREE_SPACE_3D over Node3D's (the 3-D map's column rectangle)."""
        self.e.check(self.e.lib.bpf_pf_set_random_pose_generator(self.e.h, int(mode)))

    def setUniformPoseCheck(self, threshold, multiplier, scoring=POSE_CHECK_AS_REFERENCE):
        """Node::uniformPoseGenerator's score check (uniform_pose_starting_weight_threshold,
        uniform_pose_deweight_multiplier); see bpf_pf_set_uniform_pose_check in include/badger_pf.h."""
        self.e.check(self.e.lib.bpf_pf_set_uniform_pose_check(self.e.h, float(threshold), float(multiplier),
                                                              int(scoring)))

    def setKldCount(self, mode):
        """KLD_COUNT_LEAVES (default, the reference's PFKDTree::getLeafCount) or KLD_COUNT_BINS (distinct histogram
        bins, as in KLD-sampling; parity unpinned by construction).  Takes effect at the next resample; in BINS mode
        every leaf count the filter reports or takes is a bin count.  See bpf_pf_set_kld_count."""
        self.e.check(self.e.lib.bpf_pf_set_kld_count(self.e.h, int(mode)))

    def getKldCount(self):
        m = C.c_int(0)
        self.e.check(self.e.lib.bpf_pf_get_kld_count(self.e.h, C.byref(m)))
        return m.value

    def setPopulationSizeParameters(self, pop_err, pop_z):
        self.e.check(self.e.lib.bpf_pf_set_population_size_parameters(self.e.h, pop_err, pop_z))

    def setDecayRates(self, alpha_slow, alpha_fast):
        self.e.check(self.e.lib.bpf_pf_set_decay_rates(self.e.h, alpha_slow, alpha_fast))

    def srand48(self, seed):
        self.e.check(self.e.lib.bpf_pf_srand48(self.e.h, seed))

    def getRngState(self):
        s = C.c_uint64()
        self.e.check(self.e.lib.bpf_pf_get_rng_state(self.e.h, C.byref(s)))
        return s.value

    def setRngState(self, state):
        self.e.check(self.e.lib.bpf_pf_set_rng_state(self.e.h, state))

    def initWithSamples(self, samples, leaf_count=-1):
        """What initWithPoseFn / initWithGaussian leave behind: poses + weights of the current set."""
        s = np.ascontiguousarray(samples, dtype=np.float64)
        assert s.ndim == 2 and s.shape[1] == 4
        self.e.check(self.e.lib.bpf_pf_set_samples(self.e.h, _dp(s), s.shape[0], leaf_count))

    def initWithGaussian(self, mean, rotation, sigma):
        """ParticleFilter::initWithGaussian given PDFGaussian's decomposition (cr_ row-major 3x3, cd_)."""
        m, r, d = (np.ascontiguousarray(v, dtype=np.float64).reshape(-1) for v in (mean, rotation, sigma))
        assert m.size == 3 and r.size == 9 and d.size == 3
        self.e.check(self.e.lib.bpf_pf_init_with_gaussian(self.e.h, _dp(m), _dp(r), _dp(d)))

    def initWithMixture(self, components):
        """The set of K Gaussian components (a MIXTURE_COMPONENT_DTYPE array, e.g. from mixtureFromHits), component k
        taking count_k consecutive samples from the filter's one drand48 stream.  Not a reference call for K > 1;
        K = 1 is initWithGaussian.  See bpf_pf_init_with_mixture in include/badger_pf.h."""
        comps, ptr = mixture_components(components)
        self.e.check(self.e.lib.bpf_pf_init_with_mixture(self.e.h, ptr, comps.shape[0]))

    def initWithRandomPoses(self):
        """ParticleFilter::initWithPoseFn with the generator of setRandomPoseGenerator (global localisation)."""
        self.e.check(self.e.lib.bpf_pf_init_with_random_poses(self.e.h))

    def initWithPoseFn(self, pose_fn):
        s = np.zeros((self.max_samples, 4), dtype=np.float64)
        for i in range(self.max_samples):
            s[i, :3] = pose_fn()
        s[:, 3] = 1.0 / self.max_samples
        self.initWithSamples(s)

    def snapshot(self):
        self.e.check(self.e.lib.bpf_pf_snapshot(self.e.h))

    def restore(self):
        self.e.check(self.e.lib.bpf_pf_restore(self.e.h))

    def fillWeights(self, w):
        self.e.check(self.e.lib.bpf_pf_fill_weights(self.e.h, w))

    def updateResample(self):
        self.e.check(self.e.lib.bpf_pf_update_resample(self.e.h))

    def getState(self):
        st = _lib.PFState()
        self.e.check(self.e.lib.bpf_pf_get_state(self.e.h, C.byref(st)))
        return st

    def getCurrentSet(self, out=None):
        """The current set copied to the host; `out` = the caller's own [max_samples, 4] buffer (e.g. the registered
        `samples` storage of a host-side set): the result is then a view of it, not a copy."""
        st = self.getState()
        mine = out is None
        if mine:
            out = np.empty((self.max_samples, 4), dtype=np.float64)
        assert out.dtype == np.float64 and out.flags.c_contiguous and out.shape[0] >= st.sample_count
        n = C.c_int()
        self.e.check(self.e.lib.bpf_pf_get_samples(self.e.h, _dp(out), out.shape[0], C.byref(n)))
        return PFSampleSet(out[:n.value].copy() if mine else out[:n.value], st)

    def getPoseArray(self, first=0, stride=1, out=None):
        """Node::publishParticleCloud's poses (node.cpp:335-357) formed on the device: [count, 7] float64 rows
        {x, y, 0, qx, qy, qz, qw} of samples first, first + stride, ...  `out`: the caller's own [>= count, 7] buffer,
        e.g. one registered with Engine.registerHostBuffer (the copy engine then writes it directly); the result is a
        view of it."""
        if out is None:
            n = self.getState().sample_count
            room = (n - first + stride - 1) // stride if stride >= 1 and 0 <= first < n else 0
            out = np.empty((max(room, 1), 7), dtype=np.float64)
        assert out.dtype == np.float64 and out.flags.c_contiguous and out.ndim == 2 and out.shape[1] == 7
        n = C.c_int()
        self.e.check(self.e.lib.bpf_pf_get_pose_array(self.e.h, int(first), int(stride), _dp(out), out.shape[0],
                                                      C.byref(n)))
        return out[:n.value]

    def isConverged(self):
        return bool(self.getState().converged)

    # ---- cluster statistics (particle_filter.cpp:505-660)
    def computeClusterStats(self):
        """Returns (cluster_count, set_mean[3], set_cov[5]); cov entries (0,0) (0,1) (1,0) (1,1) (2,2)."""
        n = C.c_int()
        mean = np.zeros(3)
        cov = np.zeros(5)
        self.e.check(self.e.lib.bpf_pf_compute_cluster_stats(self.e.h, C.byref(n), _dp(mean), _dp(cov)))
        return n.value, mean, cov

    def getClusterStats(self, cidx):
        """ParticleFilter::getClusterStats: (weight, mean) or None when cidx is past the last cluster."""
        c = _lib.Cluster()
        rc = self.e.lib.bpf_pf_get_cluster(self.e.h, int(cidx), C.byref(c))
        if rc == 1:  # BPF_ERR_INVALID_ARGUMENT
            return None
        self.e.check(rc)
        return c.weight, np.array(c.mean[:]), c.count, np.array(c.cov[:])

    def getMaxWeightPose(self):
        """Node2D::getMaxWeightPose (node_2d.cpp:588-617): (max_weight, pose)."""
        w = C.c_double()
        pose = np.zeros(3)
        self.e.check(self.e.lib.bpf_pf_get_max_weight_pose(self.e.h, C.byref(w), _dp(pose)))
        return w.value, pose


ODOM_MODEL_DIFF, ODOM_MODEL_OMNI, ODOM_MODEL_DIFF_CORRECTED, ODOM_MODEL_OMNI_CORRECTED, ODOM_MODEL_GAUSSIAN = range(5)


class OdomData:
    """include/amcl/sensors/odom.h:43-52."""

    def __init__(self, pose, delta, absolute_motion=None):
        self.pose = np.ascontiguousarray(pose, dtype=np.float64)
        self.delta = np.ascontiguousarray(delta, dtype=np.float64)
        # Node::updateOdom passes the delta when the odometry integrator is off (node.cpp:1083-1087)
        self.absolute_motion = np.ascontiguousarray(delta if absolute_motion is None else absolute_motion,
                                                    dtype=np.float64)


class Odom:
    """Odom sensor (src/amcl/sensors/odom.cpp): setModel + updateAction on the resident set."""

    def __init__(self, engine):
        self.e = engine

    def setModel(self, model_type, alpha1, alpha2, alpha3, alpha4, alpha5=0.0):
        self.e.check(self.e.lib.bpf_odom_set_model(self.e.h, int(model_type), alpha1, alpha2, alpha3, alpha4, alpha5))

    def updateAction(self, pf, data):
        self.e.check(self.e.lib.bpf_pf_update_action(self.e.h, _dp(data.pose), _dp(data.delta),
                                                     _dp(data.absolute_motion)))
        return True

    def updateActionShard(self, data, global_first, global_count):
        self.e.check(self.e.lib.bpf_shard_update_action(self.e.h, _dp(data.pose), _dp(data.delta),
                                                        _dp(data.absolute_motion), int(global_first),
                                                        int(global_count)))
        return True


class PlanarScanner:
    """include/amcl/sensors/planar_scanner.h:57-168"""

    def __init__(self, engine):
        self.e = engine
        self.max_beams = 0
        self.map = None
        engine.check(engine.lib.bpf_planar_set_map_factors(engine.h, 1.0, 1.0, 0.0))

    def init(self, max_beams, occupancy_map):
        self.max_beams = max_beams
        self.map = occupancy_map
        occupancy_map.upload()
        self.e.check(self.e.lib.bpf_planar_init(self.e.h, max_beams))

    def setModelBeam(self, z_hit, z_short, z_max, z_rand, sigma_hit, lambda_short):
        self.map.upload()
        self.e.check(self.e.lib.bpf_planar_set_model_beam(self.e.h, z_hit, z_short, z_max, z_rand, sigma_hit,
                                                          lambda_short))

    def setModelLikelihoodField(self, z_hit, z_rand, sigma_hit, max_distance_to_object):
        self.map.upload()
        self.e.check(self.e.lib.bpf_planar_set_model_likelihood_field(self.e.h, z_hit, z_rand, sigma_hit,
                                                                      max_distance_to_object))

    def setModelLikelihoodFieldProb(self, z_hit, z_rand, sigma_hit, max_distance_to_object, do_beamskip,
                                    beam_skip_distance, beam_skip_threshold, beam_skip_error_threshold):
        self.map.upload()
        self.e.check(self.e.lib.bpf_planar_set_model_likelihood_field_prob(
            self.e.h, z_hit, z_rand, sigma_hit, max_distance_to_object, int(do_beamskip), beam_skip_distance,
            beam_skip_threshold, beam_skip_error_threshold))

    def setModelLikelihoodFieldGompertz(self, z_hit, z_rand, sigma_hit, max_distance_to_object, gompertz_a,
                                        gompertz_b, gompertz_c, input_shift, input_scale, output_shift):
        self.map.upload()
        self.e.check(self.e.lib.bpf_planar_set_model_likelihood_field_gompertz(
            self.e.h, z_hit, z_rand, sigma_hit, max_distance_to_object, gompertz_a, gompertz_b, gompertz_c,
            input_shift, input_scale, output_shift))

    def setMapFactors(self, off_map_factor, non_free_space_factor, non_free_space_radius):
        self.e.check(self.e.lib.bpf_planar_set_map_factors(self.e.h, off_map_factor, non_free_space_factor,
                                                           non_free_space_radius))

    def setPlanarScannerPose(self, scanner_pose):
        p = np.ascontiguousarray(scanner_pose, dtype=np.float64)
        self.e.check(self.e.lib.bpf_planar_set_scanner_pose(self.e.h, _dp(p)))

    def updateSensor(self, pf, data):
        """PlanarScanner::updateSensor(pf, data): false (and no effect) when max_beams < 2."""
        if self.max_beams < 2:
            return False
        rp, ap = data.pointers()
        self.e.check(self.e.lib.bpf_pf_update_sensor_planar(self.e.h, rp, ap, data.range_count_, data.range_max_))
        return True

    def applyModelToSampleSet(self, data, samples, set_converged=0):
        """Seam A with host buffers: samples [N,4] float64, weights multiplied in place; returns total."""
        assert samples.dtype == np.float64 and samples.flags.c_contiguous
        status = C.c_int(0)
        total = self.e.lib.bpf_planar_apply_model_to_sample_set(
            self.e.h, _dp(samples), samples.shape[0], int(set_converged), _dp(data.ranges_), _dp(data.angles_),
            data.range_count_, data.range_max_, C.byref(status))
        if status.value != 0:
            self.e.check(status.value)
        return total

    def searchSpace(self, headings, cell_stride=1):
        """(candidates, free cells) of searchPoses for the current map and non_free_space_radius:
        candidates = free cells kept by cell_stride x headings, what a caller splits into ranges."""
        if self.map is not None:
            self.map.upload()
        total, cells = C.c_longlong(), C.c_int()
        self.e.check(self.e.lib.bpf_planar_search_space(self.e.h, int(headings), int(cell_stride), C.byref(total),
                                                        C.byref(cells)))
        return total.value, cells.value

    def searchPoses(self, data, headings, cell_stride, k, first=0, count=-1):
        """NOT a reference method: every free cell (every cell_stride-th in i and j) at `headings` headings scored
        against `data` on the device, the best k of candidates first .. first + count - 1 as a POSE_HIT_DTYPE array
        (score descending, equal scores by candidate).  See bpf_planar_search_poses in include/badger_pf.h."""
        if self.map is not None:
            self.map.upload()
        hits = np.zeros(max(int(k), 1), dtype=POSE_HIT_DTYPE)
        n = C.c_int()
        rp, ap = data.pointers()
        self.e.check(self.e.lib.bpf_planar_search_poses(
            self.e.h, rp, ap, data.range_count_, data.range_max_, int(headings), int(cell_stride), int(first),
            int(count), int(k), hits.ctypes.data_as(C.POINTER(_lib.PoseHit)), C.byref(n)))
        return hits[:n.value]

    def searchPosesJoint(self, datas, offsets, headings, cell_stride, k, first=0, count=-1):
        """NOT a reference method: searchPoses over several scans.  Scan s (datas[s], a PlanarData) is scored at the
        candidate's pose composed with offsets[s] = (dx, dy, dth), the weight carried from scan to scan; the rows carry
        the candidate's BASE pose.  See bpf_planar_search_poses_joint in include/badger_pf.h."""
        if self.map is not None:
            self.map.upload()
        s = len(datas)
        off = _joint_offsets(offsets, s)
        hits = np.zeros(max(int(k), 1), dtype=POSE_HIT_DTYPE)
        n = C.c_int()
        dpp = C.POINTER(C.c_double) * max(s, 1)
        ptrs = [d.pointers() for d in datas]
        counts = np.array([d.range_count_ for d in datas] + [0], dtype=np.int32)
        maxes = np.array([d.range_max_ for d in datas] + [0.0], dtype=np.float64)
        self.e.check(self.e.lib.bpf_planar_search_poses_joint(
            self.e.h, s, dpp(*[p[0] for p in ptrs]), dpp(*[p[1] for p in ptrs]),
            counts.ctypes.data_as(C.POINTER(C.c_int)), _dp(maxes), _dp(off), int(headings), int(cell_stride),
            int(first), int(count), int(k), hits.ctypes.data_as(C.POINTER(_lib.PoseHit)), C.byref(n)))
        return hits[:n.value]

    def searchJointPoses(self, offsets, headings, cell_stride, candidates):
        """The composed poses searchPosesJoint scores, [n, S, 3] float64, of the candidate indices given: formed by
        the search's own kernel (bpf_planar_search_joint_poses)."""
        if self.map is not None:
            self.map.upload()
        return _joint_poses(self.e, self.e.lib.bpf_planar_search_joint_poses, offsets, headings, cell_stride,
                            candidates)

    def searchBlocks(self, cell_stride=1, block=POSE_SEARCH_BLOCK):
        """Blocks of block x block cells that hold an entry of the strided free list: what a caller of
        searchPosesPruned splits into ranges."""
        if self.map is not None:
            self.map.upload()
        n = C.c_int()
        self.e.check(self.e.lib.bpf_planar_search_blocks(self.e.h, int(cell_stride), int(block), C.byref(n)))
        return n.value

    def searchPosesPruned(self, data, headings, cell_stride, k, block=POSE_SEARCH_BLOCK, first_block=0,
                          block_count=-1, stats=False):
        """NOT a reference method: the rows of searchPoses over the candidates whose cells lie in blocks first_block
        .. first_block + block_count - 1 of the block list, bit for bit, from fewer exact evaluations (likelihood
        field and Gompertz only).  stats=True: (hits, dict of the bpf_pose_search_stats fields).  See
        bpf_planar_search_poses_pruned in include/badger_pf.h."""
        if self.map is not None:
            self.map.upload()
        hits = np.zeros(max(int(k), 1), dtype=POSE_HIT_DTYPE)
        n = C.c_int()
        st = _lib.PoseSearchStats()
        rp, ap = data.pointers()
        self.e.check(self.e.lib.bpf_planar_search_poses_pruned(
            self.e.h, rp, ap, data.range_count_, data.range_max_, int(headings), int(cell_stride), int(block),
            int(first_block), int(block_count), int(k), hits.ctypes.data_as(C.POINTER(_lib.PoseHit)), C.byref(n),
            C.byref(st)))
        if stats:
            return hits[:n.value], {name: getattr(st, name) for name, _ in _lib.PoseSearchStats._fields_}
        return hits[:n.value]

    def searchPooledLUT(self, block=POSE_SEARCH_BLOCK):
        """(tiles, ltx, lty): the min-pooled LUT image searchPosesPruned bounds with, uint16 codes (level * 8) in the
        engine's 8x8-tiled layout.  For diagnosis and tests."""
        if self.map is not None:
            self.map.upload()
        n, ltx, lty = C.c_longlong(), C.c_int(), C.c_int()
        self.e.check(self.e.lib.bpf_planar_search_pooled_lut(self.e.h, int(block), None, 0, C.byref(n),
                                                             C.byref(ltx), C.byref(lty)))
        out = np.zeros(n.value, dtype=np.uint16)
        self.e.check(self.e.lib.bpf_planar_search_pooled_lut(
            self.e.h, int(block), out.ctypes.data_as(C.POINTER(C.c_ushort)), n.value, C.byref(n), C.byref(ltx),
            C.byref(lty)))
        return out, ltx.value, lty.value

    def searchBounds(self, data, headings, cell_stride, block=POSE_SEARCH_BLOCK, first_q=0, count=-1):
        """The upper bounds searchPosesPruned prunes with, as a float64 array: block candidate q = block_index *
        headings + h, first_q .. first_q + count - 1.  For diagnosis and tests."""
        if self.map is not None:
            self.map.upload()
        if count < 0:
            count = self.searchBlocks(cell_stride, block) * int(headings) - int(first_q)
        out = np.zeros(max(int(count), 1), dtype=np.float64)
        rp, ap = data.pointers()
        self.e.check(self.e.lib.bpf_planar_search_bounds(
            self.e.h, rp, ap, data.range_count_, data.range_max_, int(headings), int(cell_stride), int(block),
            int(first_q), int(count), out.ctypes.data_as(C.POINTER(C.c_double))))
        return out[:max(int(count), 0)]

    def refinePoses(self, data, poses, xy_radius, xy_step, theta_radius, theta_step, levels, trace=False):
        """NOT a reference method: coarse-to-fine lattice descent around every pose of `poses` (an [n, 3] array or a
        POSE_HIT_DTYPE array) against `data`, on the device.  Returns a POSE_REFINED_DTYPE array in the input order,
        with trace=True also the [n, levels] int32 array of the lattice points chosen.  See bpf_planar_refine_poses
        in include/badger_pf.h."""
        if self.map is not None:
            self.map.upload()
        rp, ap = data.pointers()
        return _refine_poses(self.e, poses, levels, trace, lambda p, n, out, tr: self.e.lib.bpf_planar_refine_poses(
            self.e.h, rp, ap, data.range_count_, data.range_max_, p, n, int(xy_radius), float(xy_step),
            int(theta_radius), float(theta_step), int(levels), out, tr))

    def poseMoments(self, data, poses, xy_radius, xy_step, theta_radius, theta_step, baseline, scores=False):
        """NOT a reference method: the score-weighted first and second moments of one refinement lattice (steps as
        given) around every pose of `poses` (an [n, 3] array, hit rows or refined rows) against `data`, on the device.
        Returns a POSE_MOMENTS_DTYPE array in the input order, with scores=True also the [n, M] lattice scores.  See
        bpf_planar_pose_moments in include/badger_pf.h."""
        if self.map is not None:
            self.map.upload()
        rp, ap = data.pointers()
        return _pose_moments(self.e, poses, xy_radius, theta_radius, scores,
                             lambda p, n, out, sp: self.e.lib.bpf_planar_pose_moments(
                                 self.e.h, rp, ap, data.range_count_, data.range_max_, p, n, int(xy_radius),
                                 float(xy_step), int(theta_radius), float(theta_step), float(baseline), out, sp))


# one row of a pose search: bpf_pose_hit
POSE_HIT_DTYPE = np.dtype([("pose", "<f8", (3,)), ("score", "<f8"), ("candidate", "<i8"), ("i", "<i4"), ("j", "<i4"),
                           ("heading", "<i4"), ("reserved", "<i4")])
assert POSE_HIT_DTYPE.itemsize == C.sizeof(_lib.PoseHit)


# one row of a pose refinement: bpf_pose_refined
POSE_REFINED_DTYPE = np.dtype([("pose", "<f8", (3,)), ("score", "<f8"), ("score_in", "<f8"), ("moved", "<i4"),
                               ("reserved", "<i4")])
assert POSE_REFINED_DTYPE.itemsize == C.sizeof(_lib.PoseRefined)


def _refine_poses(engine, poses, levels, trace, call):
    """the marshalling both scanners' refinePoses share: call(poses*, n, rows*, trace* or None) -> status"""
    poses = np.asarray(poses)
    if poses.dtype == POSE_HIT_DTYPE:
        poses = poses["pose"]
    xyt = np.ascontiguousarray(poses, dtype=np.float64).reshape(-1, 3)
    n = xyt.shape[0]
    rows = np.zeros(max(n, 1), dtype=POSE_REFINED_DTYPE)
    tr = np.zeros((max(n, 1), max(int(levels), 1)), dtype=np.int32) if trace else None
    engine.check(call(_dp(xyt), n, rows.ctypes.data_as(C.POINTER(_lib.PoseRefined)),
                      tr.ctypes.data_as(C.POINTER(C.c_int)) if trace else None))
    return (rows[:n], tr[:n]) if trace else rows[:n]


# one row of pose moments: bpf_pose_moments
POSE_MOMENTS_DTYPE = _lib.POSE_MOMENTS_DTYPE
MOMENTS_VALID, MOMENTS_FACE_X, MOMENTS_FACE_Y, MOMENTS_FACE_THETA = 1, 2, 4, 8


def _pose_moments(engine, poses, xy_radius, theta_radius, scores, call):
    """the marshalling both scanners' poseMoments share: call(poses*, n, rows*, scores* or None) -> status"""
    poses = np.asarray(poses)
    if poses.dtype.names and "pose" in poses.dtype.names:  # hit rows and refined rows alike
        poses = poses["pose"]
    xyt = np.ascontiguousarray(poses, dtype=np.float64).reshape(-1, 3)
    n = xyt.shape[0]
    rows = np.zeros(max(n, 1), dtype=POSE_MOMENTS_DTYPE)
    sc = None
    if scores:
        side, turns = 2 * max(int(xy_radius), 0) + 1, 2 * max(int(theta_radius), 0) + 1
        sc = np.zeros((max(n, 1), min(side * side * turns, 2048)), dtype=np.float64)
    engine.check(call(_dp(xyt), n, rows.ctypes.data_as(C.POINTER(_lib.PoseMoments)), _dp(sc) if scores else None))
    return (rows[:n], sc[:n]) if scores else rows[:n]


def mixtureApplyMoments(mixture, moments, sigma_floor, sigma_cap, take_mean=False):
    """The rotation and sigma (with take_mean also the mean) of every component of `mixture` -- what mixtureFromHits
    returned: (components, source_row, merged) -- from the row of `moments` (POSE_MOMENTS_DTYPE, one per hit row) it
    came from: eigenvectors and clamped eigenvalues of the row's covariance.  A component whose row is invalid keeps
    what it had.  Returns a new component array.  Plain host code, needs no GPU.  See
    bpf_pose_mixture_apply_moments in include/badger_pf.h."""
    comps = np.array(mixture[0], dtype=MIXTURE_COMPONENT_DTYPE).reshape(-1)
    src = np.ascontiguousarray(mixture[1], dtype=np.int32).reshape(-1)
    assert src.shape[0] == comps.shape[0]
    rows = np.ascontiguousarray(moments, dtype=POSE_MOMENTS_DTYPE).reshape(-1)
    lo = np.ascontiguousarray(sigma_floor, dtype=np.float64).reshape(-1)
    hi = np.ascontiguousarray(sigma_cap, dtype=np.float64).reshape(-1)
    assert lo.size == 3 and hi.size == 3
    rc = _lib.load().bpf_pose_mixture_apply_moments(
        comps.ctypes.data_as(C.POINTER(_lib.MixtureComponent)), comps.shape[0],
        src.ctypes.data_as(C.POINTER(C.c_int)), rows.ctypes.data_as(C.POINTER(_lib.PoseMoments)), rows.shape[0],
        _dp(lo), _dp(hi), 1 if take_mean else 0)
    if rc != 0:
        raise BpfError(rc, _lib.load().bpf_error_string(rc).decode())
    return comps


def pose_refine_lattice(xy_radius, theta_radius):
    """(M, m_c): the number of points and the centre's index of a refinement lattice (needs no GPU)."""
    m, c = C.c_int(), C.c_int()
    rc = _lib.load().bpf_pose_refine_lattice(int(xy_radius), int(theta_radius), C.byref(m), C.byref(c))
    if rc != 0:
        raise BpfError(rc, _lib.load().bpf_error_string(rc).decode())
    return m.value, c.value


# one component of a mixture initialiser: bpf_mixture_component
MIXTURE_COMPONENT_DTYPE = _lib.MIXTURE_COMPONENT_DTYPE


def mixture_components(components):
    """(array, pointer) of a component table as the library takes it; the array keeps the memory alive."""
    comps = np.ascontiguousarray(components, dtype=MIXTURE_COMPONENT_DTYPE).reshape(-1)
    return comps, comps.ctypes.data_as(C.POINTER(_lib.MixtureComponent))


def mixtureFromHits(rows, total_count, xy_merge, theta_merge, max_components, sigma):
    """Mixture components from pose-search hits (POSE_HIT_DTYPE) or refined rows (POSE_REFINED_DTYPE): the best rows by
    score, rows within the merge distances of a better one suppressed, total_count samples shared out by score
    (largest remainder).  Returns (components, source_row, merged): a MIXTURE_COMPONENT_DTYPE array for
    initWithMixture, the row each component came from and the rows each one suppressed.  Plain host code, needs no
    GPU.  See bpf_pose_mixture_from_hits in include/badger_pf.h."""
    rows = np.asarray(rows)
    xyt = np.ascontiguousarray(rows["pose"], dtype=np.float64).reshape(-1, 3)
    scores = np.ascontiguousarray(rows["score"], dtype=np.float64).reshape(-1)
    sg = np.ascontiguousarray(sigma, dtype=np.float64).reshape(-1)
    assert sg.size == 3
    cap = max(int(max_components), 1)
    out = np.zeros(cap, dtype=MIXTURE_COMPONENT_DTYPE)
    src = np.zeros(cap, dtype=np.int32)
    merged = np.zeros(cap, dtype=np.int32)
    n = C.c_int()
    ip = C.POINTER(C.c_int)
    rc = _lib.load().bpf_pose_mixture_from_hits(_dp(xyt), _dp(scores), xyt.shape[0], int(total_count),
                                                float(xy_merge), float(theta_merge), int(max_components), _dp(sg),
                                                out.ctypes.data_as(C.POINTER(_lib.MixtureComponent)),
                                                src.ctypes.data_as(ip), merged.ctypes.data_as(ip), C.byref(n))
    if rc != 0:
        raise BpfError(rc, _lib.load().bpf_error_string(rc).decode())
    return out[:n.value], src[:n.value], merged[:n.value]


def pose_search_window():
    """Candidates a pose search scores per window (an internal constant; needs no GPU)."""
    return int(_lib.load().bpf_pose_search_window())


def pose_search_heading_table(headings):
    """(cos, sin) of the `headings` headings of a pose search, float64 arrays: the table the joint searches compose
    their poses with (the C library's cos / sin; needs no GPU)."""
    h = int(headings)
    c, s = np.zeros(max(h, 1), dtype=np.float64), np.zeros(max(h, 1), dtype=np.float64)
    rc = _lib.load().bpf_pose_search_heading_table(h, _dp(c), _dp(s))
    if rc != 0:
        raise BpfError(rc, _lib.load().bpf_error_string(rc).decode())
    return c[:h], s[:h]


def _joint_offsets(offsets, n_scans):
    """[S, 3] float64 offsets of a joint search, one (dx, dy, dth) per scan (one spare row, so that an empty list
    still has an address)"""
    off = np.ascontiguousarray(offsets, dtype=np.float64).reshape(-1, 3)
    if off.shape[0] != n_scans:
        raise ValueError("one offset (dx, dy, dth) per scan is needed")
    return np.ascontiguousarray(np.vstack([off, np.zeros((1, 3))]))


def _joint_poses(engine, call, offsets, headings, cell_stride, candidates):
    """the marshalling both scanners' searchJointPoses share"""
    off = np.ascontiguousarray(offsets, dtype=np.float64).reshape(-1, 3)
    s = off.shape[0]
    c = np.ascontiguousarray(candidates, dtype=np.int64).reshape(-1)
    out = np.zeros((max(c.shape[0], 1), max(s, 1), 3), dtype=np.float64)
    engine.check(call(engine.h, int(headings), int(cell_stride), _dp(_joint_offsets(off, s)), s,
                      c.ctypes.data_as(C.POINTER(C.c_longlong)), c.shape[0], _dp(out)))
    return out[:c.shape[0], :s]


def merge_pose_hits(lists, k):
    """The best k rows of the hit lists of disjoint candidate ranges, in searchPoses' order (plain host code)."""
    lists = [np.ascontiguousarray(h, dtype=POSE_HIT_DTYPE) for h in lists]
    flat = np.concatenate(lists) if lists else np.zeros(0, dtype=POSE_HIT_DTYPE)
    flat = np.ascontiguousarray(flat)
    lengths = np.array([h.shape[0] for h in lists] + [0], dtype=np.int32)
    out = np.zeros(max(int(k), 1), dtype=POSE_HIT_DTYPE)
    n = C.c_int()
    rc = _lib.load().bpf_pose_search_merge(flat.ctypes.data_as(C.POINTER(_lib.PoseHit)),
                                           lengths.ctypes.data_as(C.POINTER(C.c_int)), len(lists), int(k),
                                           out.ctypes.data_as(C.POINTER(_lib.PoseHit)), C.byref(n))
    if rc != 0:
        raise BpfError(rc, _lib.load().bpf_error_string(rc).decode())
    return out[:n.value]


# --------------------------------------------------------------------------------- 3-D
class OctoMap:
    """LUT state of the reference OctoMap (include/amcl/map/octomap.h:96-110): pose_indices_,
    distance_ratios_, cropped min/max cells.  Building it from an octree is the caller's job."""

    def __init__(self, engine, resolution):
        self.e = engine
        self.resolution = float(resolution)

    def setDistancesLUT(self, pose_indices, distance_ratios, min_cells, max_cells, max_distance_to_object):
        pi = np.ascontiguousarray(pose_indices, dtype=np.uint32)
        dr = np.ascontiguousarray(distance_ratios, dtype=np.uint8)
        mn = np.ascontiguousarray(min_cells, dtype=np.int32)
        mx = np.ascontiguousarray(max_cells, dtype=np.int32)
        self.max_distance_to_object = float(max_distance_to_object)
        self.e.check(self.e.lib.bpf_map3d_set(self.e.h, pi.ctypes.data_as(C.POINTER(C.c_uint32)), pi.size,
                                              dr.ctypes.data_as(C.POINTER(C.c_uint8)), dr.size,
                                              mn.ctypes.data_as(C.POINTER(C.c_int)),
                                              mx.ctypes.data_as(C.POINTER(C.c_int)), self.resolution,
                                              self.max_distance_to_object))

    def updateDistancesLUT(self, occupied_ijk, min_cells, max_cells, max_distance_to_object):
        """OctoMap::updateDistancesLUT (octomap.cpp:175-333) from the occupied voxel indices (octree leaf order)."""
        occ = np.ascontiguousarray(occupied_ijk, dtype=np.int32).reshape(-1, 3)
        mn = np.ascontiguousarray(min_cells, dtype=np.int32)
        mx = np.ascontiguousarray(max_cells, dtype=np.int32)
        self.max_distance_to_object = float(max_distance_to_object)
        self.e.check(self.e.lib.bpf_map3d_build_distances_lut(
            self.e.h, occ.ctypes.data_as(C.POINTER(C.c_int)), occ.shape[0], mn.ctypes.data_as(C.POINTER(C.c_int)),
            mx.ctypes.data_as(C.POINTER(C.c_int)), self.resolution, self.max_distance_to_object))

    def getDistancesLUT(self):
        """(pose_indices uint32, distance_ratios uint8) as held on the device."""
        npi, ndr = C.c_size_t(), C.c_size_t()
        self.e.check(self.e.lib.bpf_map3d_get_distances_lut(self.e.h, None, 0, C.byref(npi), None, 0, C.byref(ndr)))
        pi = np.zeros(npi.value, dtype=np.uint32)
        dr = np.zeros(ndr.value, dtype=np.uint8)
        self.e.check(self.e.lib.bpf_map3d_get_distances_lut(
            self.e.h, pi.ctypes.data_as(C.POINTER(C.c_uint32)), pi.size, None,
            dr.ctypes.data_as(C.POINTER(C.c_uint8)), dr.size, None))
        return pi, dr


class PointCloudData:
    """include/amcl/sensors/point_cloud_scanner.h:45-51 (points_ as packed float xyz)"""

    def __init__(self, points_xyz):
        self.points_ = np.ascontiguousarray(points_xyz, dtype=np.float32).reshape(-1, 3)


class PointCloudScanner:
    """include/amcl/sensors/point_cloud_scanner.h:53-120"""

    def __init__(self, engine):
        self.e = engine
        self.max_beams = 0

    def init(self, max_beams, octomap):
        self.max_beams = max_beams
        self.map = octomap
        self.e.check(self.e.lib.bpf_cloud_init(self.e.h, max_beams))

    def setPointCloudModel(self, z_hit, z_rand, sigma_hit):
        self.e.check(self.e.lib.bpf_cloud_set_model(self.e.h, z_hit, z_rand, sigma_hit))

    def setPointCloudModelGompertz(self, z_hit, z_rand, sigma_hit, gompertz_a, gompertz_b, gompertz_c, input_shift,
                                   input_scale, output_shift):
        self.e.check(self.e.lib.bpf_cloud_set_model_gompertz(self.e.h, z_hit, z_rand, sigma_hit, gompertz_a,
                                                             gompertz_b, gompertz_c, input_shift, input_scale,
                                                             output_shift))

    def setMapFactors(self, off_map_factor, non_free_space_factor, non_free_space_radius):
        self.e.check(self.e.lib.bpf_cloud_set_map_factors(self.e.h, off_map_factor, non_free_space_factor,
                                                          non_free_space_radius))

    def setPointCloudScannerToFootprintTF(self, xyz, quat_xyzw):
        t = np.ascontiguousarray(xyz, dtype=np.float64)
        q = np.ascontiguousarray(quat_xyzw, dtype=np.float64)
        self.e.check(self.e.lib.bpf_cloud_set_scanner_to_footprint_tf(self.e.h, _dp(t), _dp(q)))

    def updateSensor(self, pf, data):
        if self.max_beams < 2:
            return False
        pts = data.points_
        self.e.check(self.e.lib.bpf_pf_update_sensor_cloud(self.e.h, pts.ctypes.data_as(C.POINTER(C.c_float)),
                                                           pts.shape[0]))
        return True

    def applyModelToSampleSet(self, data, samples):
        assert samples.dtype == np.float64 and samples.flags.c_contiguous
        status = C.c_int(0)
        pts = data.points_
        total = self.e.lib.bpf_cloud_apply_model_to_sample_set(self.e.h, _dp(samples), samples.shape[0],
                                                               pts.ctypes.data_as(C.POINTER(C.c_float)),
                                                               pts.shape[0], C.byref(status))
        if status.value != 0:
            self.e.check(status.value)
        return total

    def searchSpace(self, headings, cell_stride=1):
        """(candidates, columns) of searchPoses for the current 3-D map: candidates = columns of
        Node3D::updateFreeSpaceIndices kept by cell_stride x headings, what a caller splits into ranges."""
        total, cols = C.c_longlong(), C.c_int()
        self.e.check(self.e.lib.bpf_cloud_search_space(self.e.h, int(headings), int(cell_stride), C.byref(total),
                                                       C.byref(cols)))
        return total.value, cols.value

    def searchPoses(self, data, headings, cell_stride, k, first=0, count=-1):
        """NOT a reference method: every column of the 3-D map's rectangle (every cell_stride-th in i and j) at
        `headings` headings scored against the cloud `data` on the device, the best k of candidates first ..
        first + count - 1 as a POSE_HIT_DTYPE array (score descending, equal scores by candidate).  See
        bpf_cloud_search_poses in include/badger_pf.h."""
        hits = np.zeros(max(int(k), 1), dtype=POSE_HIT_DTYPE)
        n = C.c_int()
        pts = data.points_
        self.e.check(self.e.lib.bpf_cloud_search_poses(
            self.e.h, pts.ctypes.data_as(C.POINTER(C.c_float)), pts.shape[0], int(headings), int(cell_stride),
            int(first), int(count), int(k), hits.ctypes.data_as(C.POINTER(_lib.PoseHit)), C.byref(n)))
        return hits[:n.value]

    def searchPosesJoint(self, datas, offsets, headings, cell_stride, k, first=0, count=-1):
        """NOT a reference method: searchPoses over several clouds.  Cloud s (datas[s], a PointCloudData) is scored
        at the candidate's pose composed with offsets[s] = (dx, dy, dth), the weight carried from cloud to cloud; the
        rows carry the candidate's BASE pose.  See bpf_cloud_search_poses_joint in include/badger_pf.h."""
        s = len(datas)
        off = _joint_offsets(offsets, s)
        hits = np.zeros(max(int(k), 1), dtype=POSE_HIT_DTYPE)
        n = C.c_int()
        fp = C.POINTER(C.c_float)
        counts = np.array([d.points_.shape[0] for d in datas] + [0], dtype=np.int32)
        self.e.check(self.e.lib.bpf_cloud_search_poses_joint(
            self.e.h, s, (fp * max(s, 1))(*[d.points_.ctypes.data_as(fp) for d in datas]),
            counts.ctypes.data_as(C.POINTER(C.c_int)), _dp(off), int(headings), int(cell_stride), int(first),
            int(count), int(k), hits.ctypes.data_as(C.POINTER(_lib.PoseHit)), C.byref(n)))
        return hits[:n.value]

    def searchJointPoses(self, offsets, headings, cell_stride, candidates):
        """The composed poses searchPosesJoint scores, [n, S, 3] float64, of the candidate indices given: formed by
        the search's own kernel (bpf_cloud_search_joint_poses)."""
        return _joint_poses(self.e, self.e.lib.bpf_cloud_search_joint_poses, offsets, headings, cell_stride,
                            candidates)

    def searchBlocks(self, cell_stride=1, block=POSE_SEARCH_CLOUD_BLOCK):
        """Blocks of block x block columns that hold a column of the strided rectangle: what a caller of
        searchPosesPruned splits into ranges."""
        n = C.c_int()
        self.e.check(self.e.lib.bpf_cloud_search_blocks(self.e.h, int(cell_stride), int(block), C.byref(n)))
        return n.value

    def searchPosesPruned(self, data, headings, cell_stride, k, block=POSE_SEARCH_CLOUD_BLOCK, first_block=0,
                          block_count=-1, stats=False):
        """NOT a reference method: the rows of searchPoses over the candidates whose columns lie in blocks first_block
        .. first_block + block_count - 1 of the block list, bit for bit, from fewer exact evaluations (a mounting
        without roll or pitch and a map with the dense volume only).  stats=True: (hits, dict of the
        bpf_pose_search_stats fields).  See bpf_cloud_search_poses_pruned in include/badger_pf.h."""
        hits = np.zeros(max(int(k), 1), dtype=POSE_HIT_DTYPE)
        n = C.c_int()
        st = _lib.PoseSearchStats()
        pts = data.points_
        self.e.check(self.e.lib.bpf_cloud_search_poses_pruned(
            self.e.h, pts.ctypes.data_as(C.POINTER(C.c_float)), pts.shape[0], int(headings), int(cell_stride),
            int(block), int(first_block), int(block_count), int(k), hits.ctypes.data_as(C.POINTER(_lib.PoseHit)),
            C.byref(n), C.byref(st)))
        if stats:
            return hits[:n.value], {name: getattr(st, name) for name, _ in _lib.PoseSearchStats._fields_}
        return hits[:n.value]

    def searchPooledLut(self, block=POSE_SEARCH_CLOUD_BLOCK):
        """(bytes, ntx, nty, planes): the min-pooled volume searchPosesPruned bounds with, uint8 distance ratios in the
        engine's dense layout (planes of ntx x nty tiles of 8 x 8, the zero plane last).  For diagnosis and tests."""
        n, ntx, nty, planes = C.c_longlong(), C.c_int(), C.c_int(), C.c_int()
        self.e.check(self.e.lib.bpf_cloud_search_pooled_lut(self.e.h, int(block), None, 0, C.byref(n), C.byref(ntx),
                                                            C.byref(nty), C.byref(planes)))
        out = np.zeros(n.value, dtype=np.uint8)
        self.e.check(self.e.lib.bpf_cloud_search_pooled_lut(
            self.e.h, int(block), out.ctypes.data_as(C.POINTER(C.c_ubyte)), n.value, C.byref(n), C.byref(ntx),
            C.byref(nty), C.byref(planes)))
        return out, ntx.value, nty.value, planes.value

    def searchBounds(self, data, headings, cell_stride, block=POSE_SEARCH_CLOUD_BLOCK, first_q=0, count=-1):
        """The upper bounds searchPosesPruned prunes with, as a float64 array: block candidate q = block_index *
        headings + h, first_q .. first_q + count - 1.  For diagnosis and tests."""
        if count < 0:
            count = self.searchBlocks(cell_stride, block) * int(headings) - int(first_q)
        out = np.zeros(max(int(count), 1), dtype=np.float64)
        pts = data.points_
        self.e.check(self.e.lib.bpf_cloud_search_bounds(
            self.e.h, pts.ctypes.data_as(C.POINTER(C.c_float)), pts.shape[0], int(headings), int(cell_stride),
            int(block), int(first_q), int(count), out.ctypes.data_as(C.POINTER(C.c_double))))
        return out[:max(int(count), 0)]

    def refinePoses(self, data, poses, xy_radius, xy_step, theta_radius, theta_step, levels, trace=False):
        """NOT a reference method: coarse-to-fine lattice descent around every pose of `poses` (an [n, 3] array or a
        POSE_HIT_DTYPE array) against the cloud `data`, on the device.  Returns a POSE_REFINED_DTYPE array in the
        input order, with trace=True also the [n, levels] int32 array of the lattice points chosen.  See
        bpf_cloud_refine_poses in include/badger_pf.h."""
        pts = data.points_
        return _refine_poses(self.e, poses, levels, trace, lambda p, n, out, tr: self.e.lib.bpf_cloud_refine_poses(
            self.e.h, pts.ctypes.data_as(C.POINTER(C.c_float)), pts.shape[0], p, n, int(xy_radius), float(xy_step),
            int(theta_radius), float(theta_step), int(levels), out, tr))

    def poseMoments(self, data, poses, xy_radius, xy_step, theta_radius, theta_step, baseline, scores=False):
        """NOT a reference method: the score-weighted first and second moments of one refinement lattice (steps as
        given) around every pose of `poses` (an [n, 3] array, hit rows or refined rows) against the cloud `data`, on
        the device.  Returns a POSE_MOMENTS_DTYPE array in the input order, with scores=True also the [n, M] lattice
        scores.  See bpf_cloud_pose_moments in include/badger_pf.h."""
        pts = data.points_
        return _pose_moments(self.e, poses, xy_radius, theta_radius, scores,
                             lambda p, n, out, sp: self.e.lib.bpf_cloud_pose_moments(
                                 self.e.h, pts.ctypes.data_as(C.POINTER(C.c_float)), pts.shape[0], p, n,
                                 int(xy_radius), float(xy_step), int(theta_radius), float(theta_step),
                                 float(baseline), out, sp))


def uniform_pose_retries(threshold, multiplier):
    """Trials every call of Node::uniformPoseGenerator rejects under POSE_CHECK_AS_REFERENCE (the reference's score
    is always 1.0); -1 when that would pass 2^30.  Needs no GPU."""
    return int(_lib.load().bpf_uniform_pose_retries(float(threshold), float(multiplier)))
