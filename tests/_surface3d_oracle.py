"""Float64 oracle of the per-scan surface-distance metrics (``functional.surface_distances_3d`` / ``VolumeSurfaceMeter``),
restated from their definition with scipy as tests/_surface_oracle.py restates the slice-wise ones: border = mask AND NOT
erosion by the 6-connected 3-D cross (outside the volume = background; in a one-slice volume every voxel of the mask), directed
distances = the exact 3-D Euclidean distance transform of the other border under ``sampling=(sz, sy, sx)`` gathered at the own
border voxels, HD / MHD / ASD as in the 2-D oracle; an empty mask raises ``RuntimeError``.  ``directed_brute`` is an independent
all-pairs formulation that adds ``((dz sz)^2 + (dy sy)^2) + (dx sx)^2`` in that order.  Also the seeded volumes the GPU tests
share; every generator puts every class into every volume."""
import numpy as np
from scipy import ndimage

from tests import _surface_oracle as O2

EPS = O2.EPS
ANISO = (5.0, 1.25, 1.5)
_CROSS = ndimage.generate_binary_structure(3, 1)
hausdorff, mod_hausdorff, average_surface = O2.hausdorff, O2.mod_hausdorff, O2.average_surface  # (take ``directed_fn``)


def _spacing(voxelspacing):
    if voxelspacing is None:
        return 1.0, 1.0, 1.0
    if isinstance(voxelspacing, (int, float)):
        return (float(voxelspacing),) * 3
    sz, sy, sx = voxelspacing
    return float(sz), float(sy), float(sx)


def border(mask):
    mask = np.asarray(mask, dtype=bool)
    assert mask.ndim == 3
    return mask & ~ndimage.binary_erosion(mask, structure=_CROSS, iterations=1, border_value=0)


def directed(a, b, voxelspacing=None):
    """for every border voxel of ``a`` (row-major order) the distance to the nearest border voxel of ``b``"""
    a, b = np.asarray(a, dtype=bool), np.asarray(b, dtype=bool)
    if not a.any():
        raise RuntimeError("The first supplied array does not contain any binary object.")
    if not b.any():
        raise RuntimeError("The second supplied array does not contain any binary object.")
    dt = ndimage.distance_transform_edt(~border(b), sampling=_spacing(voxelspacing))
    return dt[border(a)]


def directed_brute(a, b, voxelspacing=None):
    """the same multiset by an all-pairs search, the three squares added as ((z + y) + x)"""
    a, b = np.asarray(a, dtype=bool), np.asarray(b, dtype=bool)
    if not a.any() or not b.any():
        raise RuntimeError("an array does not contain any binary object.")
    sz, sy, sx = _spacing(voxelspacing)
    p, q = np.argwhere(border(a)).astype(np.float64), np.argwhere(border(b)).astype(np.float64)
    out = np.empty(len(p))
    for i0 in range(0, len(p), 512):  # (in blocks: the all-pairs table of a dense volume would not fit)
        dz = (p[i0:i0 + 512, None, 0] - q[None, :, 0]) * sz
        dy = (p[i0:i0 + 512, None, 1] - q[None, :, 1]) * sy
        dx = (p[i0:i0 + 512, None, 2] - q[None, :, 2]) * sx
        out[i0:i0 + 512] = np.sqrt((dz * dz + dy * dy) + dx * dx).min(axis=1)
    return out


def surface_distances(pred, target, C, report_axis=None, voxelspacing=None, percentile=95.0):
    """class-coded [V,D,H,W] (or [D,H,W]) maps -> dict of [V, n_report] arrays: hd, mhd, asd (NaN where empty), empty (bool),
    n (the larger border-voxel count of the pair)"""
    pred, target = np.asarray(pred), np.asarray(target)
    if pred.ndim == 3:
        pred, target = pred[None], target[None]
    report = list(range(C)) if report_axis is None else list(report_axis)
    V = pred.shape[0]
    out = {k: np.full((V, len(report)), np.nan) for k in ("hd", "mhd", "asd")}
    out["empty"] = np.zeros((V, len(report)), dtype=bool)
    out["n"] = np.zeros((V, len(report)), dtype=np.int64)
    for v in range(V):
        for r, c in enumerate(report):
            a, t = pred[v] == c, target[v] == c
            if not a.any() or not t.any():
                out["empty"][v, r] = True
                continue
            d_at, d_ta = directed(a, t, voxelspacing), directed(t, a, voxelspacing)
            out["hd"][v, r] = max(d_at.max(), d_ta.max())
            out["mhd"][v, r] = max(np.percentile(d_at, percentile), np.percentile(d_ta, percentile))
            out["asd"][v, r] = (d_at.mean() + d_ta.mean()) / 2.0
            out["n"][v, r] = max(d_at.size, d_ta.size)
    return out


def meter(scans, C, report_axis, metername, voxelspacing=None):
    """``VolumeSurfaceMeter`` over (pred, target) scans of shape [D,H,W]: a scan in which a reported class is missing from
    the whole volume of either map is dropped -> (mean, std, skipped scans, rows)"""
    key = {"hausdorff": "hd", "mod_hausdorff": "mhd", "average_surface": "asd"}[metername]
    rows, skipped = [], 0
    for pred, target in scans:
        o = surface_distances(pred, target, C, report_axis, voxelspacing, 95.0)
        if o["empty"].any():
            skipped += 1
        else:
            rows.append(o[key])
    if not rows:
        nan = np.full(len(report_axis), np.nan)
        return nan, nan, skipped, np.zeros((0, len(report_axis)))
    rows = np.concatenate(rows, 0)
    return rows.mean(0), rows.std(0), skipped, rows


# ---- seeded volumes
def blob_volumes(V, D, H, W, C, seed):
    """class-coded [V,D,H,W] map: arg-max of C smoothed 3-D noise fields (the 3-D analogue of ``blob_maps``, seeded the same
    way); every class 0 .. C-1 is present in every volume (needs D * H * W >= C)"""
    n = D * H * W
    assert n >= C
    rng = np.random.RandomState(seed)
    out = np.zeros((V, D, H, W), dtype=np.int64)
    sigma = (max(0.6, D / 8.0), max(0.6, min(H, W) / 8.0), max(0.6, min(H, W) / 8.0))
    for v in range(V):
        fields = np.stack([ndimage.gaussian_filter(rng.randn(D, H, W), sigma=sigma, mode="nearest") for _ in range(C)])
        m = fields.argmax(0).reshape(-1)
        for _ in range(2 * C):  # stamp a voxel of every missing class (a stamp may remove another class's last voxel: repeat)
            missing = [c for c in range(C) if not (m == c).any()]
            if not missing:
                break
            for c in missing:
                m[(c * (n // C) + rng.randint(0, max(1, n // C))) % n] = c
        assert all((m == c).any() for c in range(C))
        out[v] = m.reshape(D, H, W)
    return out


def random_volumes(V, D, H, W, C, seed):
    """per-voxel uniform random labels (``random_maps`` of D slices per volume): nearly every voxel is a border voxel"""
    out = O2.random_maps(V * D, H, W, C, seed).reshape(V, D, H, W)
    assert all((out[v] == c).any() for v in range(V) for c in range(C))
    return out


def tiny_volumes(V, D, H, W, seed):
    """two-class maps for the degenerate shapes: random bits, class 1 present in every volume of both maps"""
    rng = np.random.RandomState(seed)
    maps = []
    for _ in range(2):
        m = (rng.rand(V, D, H, W) < 0.4).astype(np.int64)
        for v in range(V):
            m[v].flat[rng.randint(D * H * W)] = 1
        maps.append(m)
    return maps


def line_against_voxel(n, start=3):
    """target: one voxel at (0, 0, 0); pred: n voxels along z from slice ``start`` at (y, x) = (0, 0) -- every one a border
    voxel, at the distinct distances start .. start + n - 1 slices; the converse directed set is the single value ``start``"""
    pred, target = np.zeros((start + n + 2, 2, 3), bool), np.zeros((start + n + 2, 2, 3), bool)
    pred[start:start + n, 0, 0], target[0, 0, 0] = True, True
    return pred, target
