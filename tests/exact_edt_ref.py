"""The capped Euclidean distance transform that updateDistancesLUTExact promises, written out directly, and maps
wider than one 256-thread block of its kernels.  An ordinary module, like map_geometry.py."""
import numpy as np


def radius_cells(max_dist, res):
    """floor(max_dist / resolution) in double, as the engine forms it."""
    return int(np.floor(float(max_dist) / float(res)))


def direct_edt(cells, res, max_dist, walk=None):
    """For every cell the minimum of a^2 + b^2 over the occupied cells (== 1) inside its (2 r + 1)^2 window, in one
    pass over (cell, occupied cell) pairs -- no separable passes; float32(sqrt(best) * res) where best <= r^2, else
    float32(max_dist).  The pairs are walked by occupied cell or by window offset (`walk` = "occupied" / "offsets"),
    whichever is fewer if it is not said."""
    sy, sx = cells.shape
    r = radius_cells(max_dist, res)
    none = np.iinfo(np.int64).max
    best = np.full((sy, sx), none, dtype=np.int64)
    occ = cells == 1
    where = np.argwhere(occ)
    if walk is None:
        walk = "occupied" if where.shape[0] <= (2 * r + 1) ** 2 else "offsets"
    if walk == "occupied":
        ys, xs = np.mgrid[0:sy, 0:sx]
        for oy, ox in where:
            y0, y1, x0, x1 = max(oy - r, 0), min(oy + r + 1, sy), max(ox - r, 0), min(ox + r + 1, sx)
            d2 = (ys[y0:y1, x0:x1] - oy) ** 2 + (xs[y0:y1, x0:x1] - ox) ** 2
            np.minimum(best[y0:y1, x0:x1], d2, out=best[y0:y1, x0:x1])
    else:
        for b in range(-min(r, sy - 1), min(r, sy - 1) + 1):
            for a in range(-min(r, sx - 1), min(r, sx - 1) + 1):
                # the cell (x, y) sees the occupied cell (x + a, y + b)
                dst = best[max(-b, 0):sy - max(b, 0), max(-a, 0):sx - max(a, 0)]
                src = occ[max(b, 0):sy - max(-b, 0), max(a, 0):sx - max(-a, 0)]
                np.minimum(dst, np.where(src, a * a + b * b, none), out=dst)
    near = best <= r * r
    return np.where(near, np.sqrt(np.where(near, best, 0).astype(np.float64)) * float(res),
                    float(max_dist)).astype(np.float32)


def seam_map(size_x, size_y, seed=0):
    """cells[int32, size_y x size_x] of a map whose long axis spans three 256-cell blocks: free, single occupied cells
    on both sides of the seams 255 | 256 and 511 | 512 of the long axis (at 1, 3, 6 and 11 cells from them, so that
    windows of every radius straddle a seam), a sparse scatter of occupied (0.3 %) and unknown (1 %) cells.  The tall
    form is the wide one transposed."""
    if size_y > size_x:
        return np.ascontiguousarray(seam_map(size_y, size_x, seed).T)
    rng = np.random.default_rng(seed)
    u = rng.random((size_y, size_x))
    cells = np.full((size_y, size_x), -1, dtype=np.int32)
    cells[u < 0.003] = 1
    cells[(u >= 0.003) & (u < 0.013)] = 0
    row = 2
    for seam in (256, 512):
        for d in (1, 3, 6, 11):
            for x in (seam - d, seam + d - 1):      # the d-th cell left of the seam and the d-th right of it
                if x < size_x:
                    cells[row % size_y, max(x - 2, 0):x + 3] = -1
                    cells[row % size_y, x] = 1
                    row += 7
    return cells
