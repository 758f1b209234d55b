"""numpy restatement of pf_cavity_fwd's contract (include/pepflow_hip.h, csrc/cavity.hip) for one structure, in two modes:

  dtype = np.float64   the definitions in double precision;
  dtype = np.float32   the kernel's arithmetic: the same operations on np.float32 values in the stated order (numpy rounds every
                       operation and never contracts), so the comparisons `<=` see the values the kernel sees.

  Point       linear index (ix * ny + iy) * nz + iz (numpy's C order of an [nx, ny, nz] array); g = origin + index * h per axis.
  Occupied    ((dx*dx + dy*dy) + dz*dz) <= R_a*R_a for some atom with its mask set, dx = gx - ax ..., R_a = radius[type, slot] + probe.
  Buriedness  of a free point: the number of the 7 lines (3 axes, 4 body diagonals) with an occupied point within n_axis / n_diag steps
              in both senses, walks ending at the grid's edge; 255 where occupied.
  Cavities    components (scipy.ndimage.label, 6- or 26-connectivity) of the free points with buriedness >= min_buried; those of at
              least min_points points, by size descending, ties by the smallest linear index; the first max_cavities are reported.
The components come from scipy, the occupancy from every atom against a generous index box in float64 (or, with brute=True, against
the whole grid) and the walks from shifted copies of the occupancy: none of it follows the kernels' way of computing.
"""
import math

import numpy as np
from scipy import ndimage

DEFAULTS = {"probe": 1.4, "max_ray": 12.0, "min_buried": 5, "connectivity": 6, "min_points": 8, "max_cavities": 8, "r_lining": 4.5}
LINES = ((1, 0, 0), (0, 1, 0), (0, 0, 1), (1, 1, 1), (1, 1, -1), (1, -1, 1), (1, -1, -1))


def steps(h, max_ray):
    """(n_axis, n_diag): computed in float64, as the caller of the kernel does"""
    return int(math.floor(max_ray / h)), int(math.floor(max_ray / (h * math.sqrt(3.0))))


def axis_coords(origin, n, h, dtype):
    """g = origin + index * h of one axis in `dtype` (float32: a rounded product and a rounded sum of float32 values)"""
    return (dtype(origin) + np.arange(n).astype(dtype) * dtype(h)).astype(dtype)


def _atoms(pos, mask, aa, radius, dtype):
    """the atoms with their mask set: (coordinates [M,3], table radius [M], residue [M]) in `dtype` (from the float32 inputs)"""
    pos, mask = np.asarray(pos, np.float32), np.asarray(mask).astype(bool)
    S = min(pos.shape[1], 15)
    res, slot = np.nonzero(mask[:, :S])
    row = np.where((np.asarray(aa) < 0) | (np.asarray(aa) > 20), 20, np.asarray(aa))[res]
    return pos[res, slot].astype(dtype), np.asarray(radius, np.float32)[row, slot].astype(dtype), res


def _shift(a, s, k):
    """a moved so that out[i] = a[i + k * s], False beyond the edge"""
    out = np.zeros_like(a)
    src, dst = [], []
    for ax in range(3):
        n, d = a.shape[ax], k * s[ax]
        if abs(d) >= n:
            return out
        src.append(slice(max(d, 0), n + min(d, 0)))
        dst.append(slice(max(-d, 0), n + min(-d, 0)))
    out[tuple(dst)] = a[tuple(src)]
    return out


def scan(pos, mask, aa, radius, origin, dims, h, dtype=np.float64, brute=False, **params):
    """-> dict: occupied [G] bool, buried [G] uint8, label [G] int32, n_found, size [K], center [K,3] float64, mean_buried [K]
    float64, lining [K,N] bool, points (list of [size,3] member coordinates in `dtype`)"""
    p = {**DEFAULTS, **params}
    nx, ny, nz = dims
    N = np.asarray(pos).shape[0]
    xyz, rad, res = _atoms(pos, mask, aa, radius, dtype)
    g = [axis_coords(origin[ax], dims[ax], h, dtype) for ax in range(3)]
    occ = np.zeros(dims, bool)
    for (ax, ay, az), r in zip(xyz, rad):
        R = dtype(r + dtype(p["probe"]))
        if brute:
            sl = (slice(0, nx), slice(0, ny), slice(0, nz))
        else:                                               # three points of slack beyond the sphere's extent, in float64
            sl = tuple(slice(max(int(math.floor((float(c) - float(R) - float(origin[k])) / h)) - 3, 0),
                             max(int(math.ceil((float(c) + float(R) - float(origin[k])) / h)) + 4, 0)) for k, c in enumerate((ax, ay, az)))
        dx, dy, dz = g[0][sl[0]] - ax, g[1][sl[1]] - ay, g[2][sl[2]] - az
        d2 = ((dx * dx)[:, None, None] + (dy * dy)[None, :, None]) + (dz * dz)[None, None, :]
        assert d2.dtype == dtype
        occ[sl] |= d2 <= R * R
    n_axis, n_diag = steps(h, p["max_ray"])
    buried = np.zeros(dims, np.int64)
    for li, s in enumerate(LINES):
        n = n_axis if li < 3 else n_diag
        both = np.ones(dims, bool)
        for sense in (1, -1):
            hit = np.zeros(dims, bool)
            for k in range(1, min(n, max(dims)) + 1):
                hit |= _shift(occ, s, sense * k)
            both &= hit
        buried += both
    buried = np.where(occ, 255, buried).astype(np.uint8)
    cav = ~occ & (buried >= p["min_buried"])
    structure = ndimage.generate_binary_structure(3, 1 if p["connectivity"] == 6 else 3)
    lab, n_comp = ndimage.label(cav, structure=structure)
    flat = lab.reshape(-1)
    sizes = np.bincount(flat, minlength=n_comp + 1)
    first = np.full(n_comp + 1, flat.size, np.int64)
    np.minimum.at(first, flat, np.arange(flat.size))
    kept = [c for c in range(1, n_comp + 1) if sizes[c] >= p["min_points"]]
    kept.sort(key=lambda c: (-sizes[c], first[c]))
    K = p["max_cavities"]
    out = {"occupied": occ.reshape(-1), "buried": buried.reshape(-1), "n_found": len(kept), "label": np.full(flat.size, -1, np.int32),
           "size": np.zeros(K, np.int32), "center": np.zeros((K, 3)), "mean_buried": np.zeros(K), "lining": np.zeros((K, N), bool),
           "points": []}
    rl = dtype(p["r_lining"])
    for k, c in enumerate(kept[:K]):
        members = flat == c
        out["label"][members] = k
        ix, iy, iz = np.nonzero(lab == c)
        pts = np.stack([g[0][ix], g[1][iy], g[2][iz]], 1)
        out["points"].append(pts)
        out["size"][k] = sizes[c]
        out["center"][k] = pts.astype(np.float64).mean(0)
        out["mean_buried"][k] = buried[ix, iy, iz].astype(np.float64).mean()
        for a0 in range(0, xyz.shape[0], 512):
            d = pts[:, None, :] - xyz[None, a0:a0 + 512, :]
            near = ((d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2] <= rl * rl).any(0)
            out["lining"][k, res[a0:a0 + 512][near]] = True
    return out


def same_partition(label_a, label_b):
    """two labelings (-1: none) split the points into the same sets, whatever the sets are called"""
    a, b = np.asarray(label_a).reshape(-1), np.asarray(label_b).reshape(-1)
    if not np.array_equal(a < 0, b < 0):
        return False
    pairs = set(zip(a[a >= 0].tolist(), b[a >= 0].tolist()))
    return len(pairs) == len({x for x, _ in pairs}) == len({y for _, y in pairs})
