"""3-D worlds for the point-cloud parity tests.  Every other cloud test scores on one world: synth.box_room_voxels()
at 0.05 m, 87 x 67 x 29 cells symmetric about cell 0.  There 1 / resolution is exact (so only the exact-reciprocal
kernels ever ran), the dense volume's tiling is never a whole number of tiles, no lower bound is positive, and z fits a
byte.  The worlds here differ in each of these; the clouds are cheap (no ray march) and reach past all six sides.

An ordinary module that the tests import, like map_geometry.py."""
import ctypes
import ctypes.util
import math
import struct

import numpy as np

from badger_amcl_amd import synth

# name -> (min cells, max cells (inclusive), resolution, 1 / resolution is exact for the kernel)
GEOMETRIES = {
    # w + 2 = 120 and h + 2 = 16: whole tiles, the far border ring is the last column of the last tile; min_x > 0
    "V1": ((3, -9, 0), (120, 4, 5), 0.1, True),
    # w + 2 = 17 (one cell into a third tile), 311 z cells (more than a byte), min_y > 0
    "V2": ((-7, 40, -150), (7, 52, 160), 0.03, False),
    # lower bounds of 10^4 cells of either sign, no span holds 0; world coordinates near 1.4 km / -2.1 km, where a
    # float ulp is 1.2e-4 m
    "V3": ((20000, -30050, 10), (20060, -30000, 30), 0.07, False),
    # a side smaller than a tile, a single z plane
    "V4": ((5, -20, 0), (7, 19, 0), 0.25, True),
    # the room of the other tests (box_room_voxels() with three cells of margin); only the resolution differs
    "V5": ((-43, -33, -5), (43, 33, 23), 0.06, False),
}

# resolutions of the voxel-rounding check (test_cloud_geometry_cpu.py)
EXACT_RESOLUTIONS = [0.05, 0.1, 0.2, 0.025, 0.04, 0.08, 0.125, 0.25, 0.5, 1.0, 0.01]
INEXACT_RESOLUTIONS = [0.03, 0.06, 0.07, 0.15, 0.3, 0.075]

TF_XYZ = (0.2, -0.1, 0.5)
MOUNT_ANGLE = 0.3
GOMPERTZ = dict(gompertz_a=0.748, gompertz_b=5.0, gompertz_c=1.2, input_shift=-3.2, input_scale=6.7,
                output_shift=0.25)
OFF_MAP_FACTOR = 0.95

# form bits of Engine.cloud_last_form() (include/badger_pf.h)
F_RAN, F_EXACT, F_PLANAR, F_DENSE, F_BORDER, F_GRADED = 32, 1, 2, 4, 8, 16

_fma = None


def fma(a, b, c):
    """libm's correctly rounded a * b + c in double."""
    global _fma
    if _fma is None:
        if hasattr(math, "fma"):
            _fma = math.fma
        else:
            m = ctypes.CDLL(ctypes.util.find_library("m") or "libm.so.6")
            m.fma.restype = ctypes.c_double
            m.fma.argtypes = [ctypes.c_double] * 3
            _fma = m.fma
    return _fma(a, b, c)


def exact_rinv(res):
    """score_cloud's rule (abi_cloud3d.inl): 1 / res has its low 24 mantissa bits clear, so that a float times it is
    exact, and rounds back onto 1."""
    rinv = 1.0 / res
    bits = struct.unpack("<Q", struct.pack("<d", rinv))[0]
    return (bits & ((1 << 24) - 1)) == 0 and abs(fma(rinv, res, -1.0)) < 1.1e-16


def voxel_reference(v, res):
    """octomap.cpp:102-107 on a float coordinate: floor(v / res + 0.5) in double, as arrays."""
    return np.floor(np.asarray(v, dtype=np.float32).astype(np.float64) / res + 0.5).astype(np.int64)


def voxel_exact_form(v, res):
    """voxel_of_exact (kernels_cloud.hpp): floor(fma(v, 1 / res, 0.5)); a list of ints."""
    rinv = 1.0 / res
    return [int(math.floor(fma(float(x), rinv, 0.5))) for x in np.asarray(v, dtype=np.float32)]


def voxel_corrected_form(v, res):
    """voxel_of: q = v r; q += fma(-q, res, v) r; floor(q + 0.5), every step rounded on its own; a list of ints."""
    rinv = 1.0 / res
    out = []
    for x in np.asarray(v, dtype=np.float32):
        d = float(x)
        q = d * rinv
        q = fma(fma(-q, res, d), rinv, q)
        out.append(int(math.floor(q + 0.5)))
    return out


def voxel1_exact_form(v, res, min_c):
    """voxel1_exact, what k_cloud_score's loop uses: the cell as cell - min + 1 by truncating fma(v, 1 / res,
    1.5 - min); an int array."""
    rinv, hm = 1.0 / res, 1.5 - float(min_c)
    return np.array([int(fma(float(x), rinv, hm)) for x in np.asarray(v, dtype=np.float32)], dtype=np.int64)


def face_floats(res, k_lo, k_hi):
    """float32((k + 0.5) res) stepped by -2 .. +2 float ulps, k = k_lo .. k_hi: [k][5] float32."""
    f = (np.arange(k_lo, k_hi + 1, dtype=np.float64) + 0.5) * res
    f = f.astype(np.float32)
    inf = np.float32(np.inf)
    m1, p1 = np.nextafter(f, -inf), np.nextafter(f, inf)
    return np.stack([np.nextafter(m1, -inf), m1, f, p1, np.nextafter(p1, inf)], axis=1)


def quat_matrix_f32(q):
    """Eigen's quaternion -> matrix formula in float, every product and sum rounded on its own (cloud_affine of the
    oracle, k_cloud_affine of the engine); q = (x, y, z, w) as doubles, narrowed first."""
    f = np.float32
    x, y, z, w = (f(v) for v in q)
    tx, ty, tz = f(2) * x, f(2) * y, f(2) * z
    twx, twy, twz = tx * w, ty * w, tz * w
    txx, txy, txz = tx * x, ty * x, tz * x
    tyy, tyz, tzz = ty * y, tz * y, tz * z
    one = f(1)
    return np.array([one - (tyy + tzz), txy - twz, txz + twy,
                     txy + twz, one - (txx + tzz), tyz - twx,
                     txz - twy, tyz + twx, one - (txx + tyy)], dtype=np.float32)


def scattered_voxels(mn, mx, count, seed):
    """`count` distinct voxels inside the bounds, from one seeded stream: no mirror or transposition symmetry."""
    rng = np.random.default_rng(seed)
    mn, mx = np.asarray(mn), np.asarray(mx)
    v = np.unique(rng.integers(mn, mx + 1, size=(4 * count, 3)), axis=0)
    return v[rng.permutation(len(v))[:count]].astype(np.int32)


class CloudScenario:
    """One named world: bounds, resolution, max_dist = 6 res, occupied voxels, the oracle's LUT, a true pose, a cloud
    in the scanner frame, 300 particles, and the two mountings of test_gpu_cloud.py (yaw only: the PLANAR kernels;
    pitched: the general kernel)."""

    def __init__(self, orc, name, n=300, n_points=5000, seed=7):
        self.orc, self.name = orc, name
        mn, mx, res, exact = GEOMETRIES[name]
        self.mn, self.mx = np.array(mn, dtype=np.int32), np.array(mx, dtype=np.int32)
        self.res, self.exact = float(res), exact
        self.max_dist = 6 * self.res
        self.sigma_hit = 2 * self.res   # neighbouring distance ratios give clearly different terms at every resolution
        self.size = (self.mx - self.mn + 1).astype(np.int64)
        self.occ = self._obstacles(seed)
        self.lut = orc.OctoMapLUT(self.mn, self.mx, self.res, self.max_dist).build(self.occ)
        a = MOUNT_ANGLE
        self.tf_xyz = TF_XYZ
        self.tf_quat = {False: (0.0, 0.0, math.sin(a / 2), math.cos(a / 2))}
        q = (0.05, 0.07, math.sin(a / 2), math.cos(a / 2))
        nq = math.sqrt(sum(v * v for v in q))
        self.tf_quat[True] = tuple(v / nq for v in q)
        # the true pose: off the middle of the map, inside a cell
        c = (self.mn + self.mx) / 2.0
        self.pose = np.array([(c[0] + 0.3) * self.res, (c[1] - 0.2) * self.res, 0.1])
        # one cloud of world points, seen through either mounting: pts[pitched]
        self.world = self._cloud(n_points, seed + 1)
        self.pts = {m: np.ascontiguousarray(self.world_to_scanner(self.world, m).astype(np.float32))
                    for m in (False, True)}
        self.samples = self._particles(n, seed + 2)

    # ------------------------------------------------------------------------------------------- construction
    def _obstacles(self, seed):
        mn, mx = self.mn, self.mx
        n_scatter = int(min(60, max(12, np.prod(self.size) // 20)))
        parts = [scattered_voxels(mn, mx, n_scatter, seed)]
        if self.name == "V5":
            parts.append(synth.box_room_voxels())
        elif self.size[2] > 1:
            # walls, floor and ceiling three cells inside the bounds (less where a side is too short for that)
            inset = np.clip((self.size - 2) // 2, 0, 3).astype(np.int32)
            parts.append(synth.box_room_voxels(tuple(int(v) for v in mn + inset), tuple(int(v) for v in mx - inset),
                                               pillar=False))
        return np.unique(np.concatenate(parts), axis=0).astype(np.int32)

    def world_to_scanner(self, world, pitched=False):
        """The inverse of `pose` composed with the mounting, in float64."""
        x, y, yaw = self.pose
        cy, sy = math.cos(yaw), math.sin(yaw)
        rz = np.array([[cy, -sy, 0.0], [sy, cy, 0.0], [0.0, 0.0, 1.0]])
        qx, qy, qz, qw = self.tf_quat[pitched]
        rm = np.array([[1 - 2 * (qy * qy + qz * qz), 2 * (qx * qy - qz * qw), 2 * (qx * qz + qy * qw)],
                       [2 * (qx * qy + qz * qw), 1 - 2 * (qx * qx + qz * qz), 2 * (qy * qz - qx * qw)],
                       [2 * (qx * qz - qy * qw), 2 * (qy * qz + qx * qw), 1 - 2 * (qx * qx + qy * qy)]])
        foot = (np.asarray(world, dtype=np.float64) - np.array([x, y, 0.0])) @ rz   # rz^T applied to rows
        return (foot - np.array(self.tf_xyz)) @ rm

    def _cloud(self, n_points, seed):
        rng = np.random.default_rng(seed)
        n_far = n_points // 10
        hit = self.occ[rng.integers(0, len(self.occ), n_points - n_far)] * self.res
        jitter = np.full(3, 0.6 * self.res)
        if self.size[2] == 1:
            jitter[2] = 0.2 * self.res   # a single plane would lose 40 % of the points to a 0.6 res jitter alone
        hit = hit + rng.normal(0.0, 1.0, hit.shape) * jitter
        lo, hi = (self.mn - 0.5) * self.res, (self.mx + 0.5) * self.res
        mid, half = (lo + hi) / 2, (hi - lo) / 2
        far = rng.uniform(mid - 1.5 * half, mid + 1.5 * half, (n_far, 3))
        return np.concatenate([hit, far])[rng.permutation(n_points)]

    def _particles(self, n, seed):
        """Inside, on and beyond the map's edges on all four sides (distances in proportion to a short side), a share
        anywhere (far outside included), a third near the true pose; yaw uniform in (-pi, pi] for half of them and
        near the true yaw or its opposite for the other half -- on a long narrow map a cloud turned anywhere leaves the
        map with nearly all its points --; three poses are not numbers."""
        rng = np.random.default_rng(seed)
        res = self.res
        lo, hi = (self.mn[:2] - 0.5) * res, (self.mx[:2] + 0.5) * res   # the map's own edges
        ext = hi - lo
        s = np.zeros((n, 4))
        side = rng.integers(0, 4, n)
        d = rng.uniform(-0.2, 0.45, n)                 # distance inside the edge (negative: off the map) ...
        along = rng.uniform(0.02, 0.98, n)
        dx, dy = d * min(ext[0], 30 * res), d * min(ext[1], 30 * res)   # ... as a share of the side, of 30 cells at most
        s[:, 0] = np.where(side == 0, hi[0] - dx, np.where(side == 1, lo[0] + dx, lo[0] + along * ext[0]))
        s[:, 1] = np.where(side == 2, hi[1] - dy, np.where(side == 3, lo[1] + dy, lo[1] + along * ext[1]))
        m = n // 8
        mid = (lo + hi) / 2
        s[:m, 0] = rng.uniform(mid[0] - 0.75 * ext[0], mid[0] + 0.75 * ext[0], m)
        s[:m, 1] = rng.uniform(mid[1] - 0.75 * ext[1], mid[1] + 0.75 * ext[1], m)
        # a third stands near the true pose, so that most of their points are on the map
        near = np.arange(n) % 3 == 1
        s[near, 0] = self.pose[0] + rng.normal(0.0, min(2.0 * res, 0.1 * ext[0]), near.sum())
        s[near, 1] = self.pose[1] + rng.normal(0.0, min(2.0 * res, 0.1 * ext[1]), near.sum())
        s[:, 2] = -rng.uniform(-np.pi, np.pi, n)       # (-pi, pi]
        half = np.arange(n) % 2 == 1
        flip = rng.integers(0, 2, n) * np.pi
        aligned = self.pose[2] + flip + rng.uniform(-1.0, 1.0, n) * min(0.2, 1.5 * ext.min() / ext.max())
        aligned = np.arctan2(np.sin(aligned), np.cos(aligned))
        s[half, 2] = aligned[half]
        s[:, 3] = rng.uniform(0.5, 1.5, n) / n
        s[n // 2, 0] = np.nan
        s[n // 2 + 5, 1] = np.inf
        s[n // 2 + 10, 2] = -np.inf
        return s

    def converged_samples(self, n, seed=4):
        """A finite set round the true pose for the resident path (resampling builds a histogram of the poses)."""
        rng = np.random.default_rng(seed)
        s = np.zeros((n, 4))
        s[:, 0] = self.pose[0] + rng.normal(0.0, 3.0 * self.res, n)
        s[:, 1] = self.pose[1] + rng.normal(0.0, 3.0 * self.res, n)
        s[:, 2] = self.pose[2] + rng.normal(0.0, 0.05, n)
        s[: n // 10, 0] += 600 * self.res   # some particles off the map
        s[:, 3] = rng.uniform(0.5, 1.5, n) / n
        return s

    # ------------------------------------------------------------------------------------------- both sides
    def oracle_cloud(self, model="plain", pitched=False, tf_xyz=None, tf_quat=None):
        orc = self.orc
        xyz = self.tf_xyz if tf_xyz is None else tf_xyz
        quat = self.tf_quat[pitched] if tf_quat is None else tf_quat
        if model == "plain":
            op = orc.cloud(orc.CLOUD_MODEL, 128, xyz, quat, z_hit=0.5, z_rand=0.05, sigma_hit=self.sigma_hit)
        else:
            op = orc.cloud(orc.CLOUD_MODEL_GOMPERTZ, 128, xyz, quat, z_hit=0.5, z_rand=0.5, sigma_hit=self.sigma_hit,
                           **GOMPERTZ)
        op.off_map_factor = OFF_MAP_FACTOR
        return op

    def gpu_scanner(self, engine, model="plain", pitched=False, tf_xyz=None, tf_quat=None, ratios=None, set_lut=True):
        """OctoMap (the oracle's LUT handed over, or with `ratios` in place of its distance ratios) and the configured
        PointCloudScanner."""
        import badger_amcl_amd as bpf
        om = bpf.OctoMap(engine, self.res)
        if set_lut:
            om.setDistancesLUT(self.lut.pose_indices, self.lut.distance_ratios if ratios is None else ratios,
                               self.lut.min_cells, self.lut.max_cells, self.max_dist)
        sc = bpf.PointCloudScanner(engine)
        sc.init(128, om)
        if model == "plain":
            sc.setPointCloudModel(0.5, 0.05, self.sigma_hit)
        else:
            g = GOMPERTZ
            sc.setPointCloudModelGompertz(0.5, 0.5, self.sigma_hit, g["gompertz_a"], g["gompertz_b"], g["gompertz_c"],
                                          g["input_shift"], g["input_scale"], g["output_shift"])
        sc.setMapFactors(OFF_MAP_FACTOR, 0.95, 0.3)
        sc.setPointCloudScannerToFootprintTF(self.tf_xyz if tf_xyz is None else tf_xyz,
                                             self.tf_quat[pitched] if tf_quat is None else tf_quat)
        return om, sc

    def full_ratios(self):
        """The LUT's ratios with 256 unreferenced bytes 0 .. 255 appended: no ratio is free, so the planar dense kernel
        takes its plain form."""
        return np.concatenate([self.lut.distance_ratios, np.arange(256, dtype=np.uint8)])

    # ------------------------------------------------------------------------------------------- what the inputs do
    def volume(self):
        """The LUT as a dense [h][w][nz] array of distance ratios."""
        w, h, nz = (int(v) for v in self.size)
        pi = self.lut.pose_indices.astype(np.int64)
        return self.lut.distance_ratios[pi[:, None] + np.arange(nz)[None, :]].reshape(h, w, nz)

    def affines(self, samples, pitched=False, tf_xyz=None, tf_quat=None):
        """R[n][9], T[n][3] in float32 as the oracle forms them (numpy's sin / cos may differ from libm's in the last
        bit: this restatement serves statistics of the inputs, and exact statements only at yaw 0)."""
        s = np.asarray(samples, dtype=np.float64)
        q_s = self.tf_quat[pitched] if tf_quat is None else tf_quat
        t_s = self.tf_xyz if tf_xyz is None else tf_xyz
        R = np.zeros((len(s), 9), dtype=np.float32)
        T = np.zeros((len(s), 3), dtype=np.float32)
        with np.errstate(all="ignore"):
            for n, (x, y, th) in enumerate(s[:, :3]):
                sh, ch = (math.sin(th / 2), math.cos(th / 2)) if math.isfinite(th) else (math.nan, math.nan)
                yq = (0.0, 0.0, sh, ch)
                q = (yq[3] * q_s[0] + yq[0] * q_s[3] + yq[1] * q_s[2] - yq[2] * q_s[1],
                     yq[3] * q_s[1] + yq[1] * q_s[3] + yq[2] * q_s[0] - yq[0] * q_s[2],
                     yq[3] * q_s[2] + yq[2] * q_s[3] + yq[0] * q_s[1] - yq[1] * q_s[0],
                     yq[3] * q_s[3] - yq[0] * q_s[0] - yq[1] * q_s[1] - yq[2] * q_s[2])
                R[n] = quat_matrix_f32(q)
                sy, cy = (math.sin(th), math.cos(th)) if math.isfinite(th) else (math.nan, math.nan)
                T[n] = (cy * t_s[0] - sy * t_s[1] + x, sy * t_s[0] + cy * t_s[1] + y, t_s[2] + 0.0)
        return R, T

    def world_points(self, samples, pts=None, **mount):
        """[n][points][3] float32: ((r0 x + r1 y) + r2 z) + t, each step rounded to float."""
        R, T = self.affines(samples, **mount)
        p = self.pts[bool(mount.get("pitched", False))] if pts is None else np.asarray(pts, dtype=np.float32)
        px, py, pz = p[None, :, 0], p[None, :, 1], p[None, :, 2]
        with np.errstate(all="ignore"):
            rows = [((R[:, 3 * r, None] * px + R[:, 3 * r + 1, None] * py) + R[:, 3 * r + 2, None] * pz) + T[:, r, None]
                    for r in range(3)]
        return np.stack(rows, axis=2)

    def cells(self, samples, pts=None, **mount):
        """[n][points][3] int64 cells relative to the lower bounds; a coordinate that is not a number lands far below
        the map, as the reference's (int)floor(NaN) does."""
        w = self.world_points(samples, pts, **mount).astype(np.float64)
        with np.errstate(all="ignore"):
            c = np.floor(w / self.res + 0.5)
        c = np.where(np.isfinite(c), c, -2.0 ** 31)
        return c.astype(np.int64) - self.mn.astype(np.int64)[None, None, :]

    def statistics(self, samples=None, pts=None, **mount):
        """dict: on (share of evaluations on the map), off[6] (evaluations past -x, +x, -y, +y, -z, +z, counted over
        particles with finite poses), seeing (share of finite particles with at least one point on the map), mostly
        (share of finite particles with more than half their points on the map), sensitive (share of on-map
        evaluations that read another ratio with the x and y cells exchanged or the z cell one higher)."""
        s = self.samples if samples is None else samples
        c = self.cells(s, pts, **mount)
        size = self.size[None, None, :]
        inside = ((c >= 0) & (c < size)).all(axis=2)
        finite = np.isfinite(s[:, :3]).all(axis=1)
        cf = c[finite]
        off = [int((cf[..., a] < 0).sum()) if lo else int((cf[..., a] >= self.size[a]).sum())
               for a in range(3) for lo in (True, False)]
        vol = self.volume()
        ci, cj, ck = (c[..., a][inside] for a in range(3))
        here = vol[cj, ci, ck]
        w, h, nz = (int(v) for v in self.size)
        sw_ok = (cj < w) & (ci < h)
        swapped = np.where(sw_ok, vol[np.minimum(ci, h - 1), np.minimum(cj, w - 1), ck], -1)
        up_ok = ck + 1 < nz
        up = np.where(up_ok, vol[cj, ci, np.minimum(ck + 1, nz - 1)], -1)
        per_particle = inside[finite].mean(axis=1)
        return dict(on=float(inside.mean()), off=off, seeing=float((per_particle > 0).mean()),
                    mostly=float((per_particle > 0.5).mean()),
                    sensitive=float(((swapped != here) | (up != here)).mean()),
                    sensitive_xy=float((swapped != here).mean()), sensitive_z=float((up != here).mean()))

    # ------------------------------------------------------------------------------------------- faces
    def face_cloud(self, axis):
        """Points for one particle at pose (0, 0, 0) under an identity mounting: the coordinate on `axis` at
        float32((k + 0.5) res) stepped by -2 .. +2 float ulps, k from five cells below the map to five above it (the
        face between cells k and k + 1), the two other coordinates at the centre of the cell where the ratios either
        side of that face differ most (off the map counts as ratio 255).  Returns (points[float32, n x 3],
        differs[bool, n]: the two voxels next to the face hold different ratios)."""
        vol = self.volume().astype(np.int64)          # [y][x][z]
        v = np.moveaxis(vol, (1, 0, 2)[axis], 0)      # axis first; the two others in y / x / z order
        pad = np.full((6,) + v.shape[1:], 255, dtype=np.int64)
        v = np.concatenate([pad, v, pad])             # cells min - 6 .. max + 6 along the axis
        step = np.abs(np.diff(v, axis=0))             # [face k = min - 6 .. max + 5]
        ks = np.arange(self.mn[axis] - 5, self.mx[axis] + 6)
        step = step[1:1 + len(ks)]
        flat = step.reshape(len(ks), -1)
        best = flat.argmax(axis=1)
        differs = flat[np.arange(len(ks)), best] > 0
        b0, b1 = np.unravel_index(best, v.shape[1:])
        others = [a for a in (1, 0, 2) if a != axis]  # the order the two remaining axes have in `v`
        f = face_floats(self.res, int(ks[0]), int(ks[-1]))
        pts = np.zeros((len(ks), 5, 3), dtype=np.float32)
        pts[:, :, axis] = f
        for b, a in zip((b0, b1), others):
            pts[:, :, a] = ((b + self.mn[a]) * self.res).astype(np.float32)[:, None]
        return np.ascontiguousarray(pts.reshape(-1, 3)), np.repeat(differs, 5)

    def robot_face_samples(self):
        """Particles whose x or y stands at (k + 0.5) res stepped by -2 .. +2 double ulps, k = min - 1, min, max,
        max + 1 (k_cloud_finish's own cell of the robot), the other coordinate mid-map."""
        rows = []
        mid = (self.mn[:2] + self.mx[:2]) / 2.0 * self.res + 0.1 * self.res
        for a in (0, 1):
            for k in (self.mn[a] - 1, self.mn[a], self.mx[a], self.mx[a] + 1):
                f = (k + 0.5) * self.res
                m1, p1 = np.nextafter(f, -np.inf), np.nextafter(f, np.inf)
                for v in (np.nextafter(m1, -np.inf), m1, f, p1, np.nextafter(p1, np.inf)):
                    row = [mid[0], mid[1], 0.3 * len(rows) - 3.0, 1.0]
                    row[a] = float(v)
                    rows.append(row)
        s = np.array(rows, dtype=np.float64)
        s[:, 3] = 1.0 / len(s)
        return s

    def robot_on_map(self, samples):
        """pose_valid3 of the robot's cell, octomap.cpp:102-107 in double."""
        c = np.floor(samples[:, :2] / self.res + 0.5)
        return ((c >= self.mn[:2]) & (c <= self.mx[:2])).all(axis=1)


_CACHE = {}


def scenario(orc, name):
    """One CloudScenario per name and process: the tests leave it unchanged."""
    if name not in _CACHE:
        _CACHE[name] = CloudScenario(orc, name)
    return _CACHE[name]
