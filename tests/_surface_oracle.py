"""Float64 oracle of the surface-distance metrics (``functional.surface_distances`` / ``SurfaceMeter``), restated from their
definition with scipy: border = mask AND NOT erosion by the 4-connected cross (outside the image = background), directed
distances = the exact Euclidean distance transform of the other border gathered at the own border pixels, HD = the larger
maximum, MHD = the larger numpy (linear) percentile, ASD = the mean of the two directed means; an empty mask raises
``RuntimeError``.  ``directed_brute`` is an independent all-pairs formulation of the same multiset.  Also the seeded maps the
GPU tests share."""
import numpy as np
from scipy import ndimage

EPS = 2.0 ** -52
_CROSS = ndimage.generate_binary_structure(2, 1)


def _spacing(voxelspacing):
    if voxelspacing is None:
        return 1.0, 1.0
    if isinstance(voxelspacing, (int, float)):
        return float(voxelspacing), float(voxelspacing)
    sy, sx = voxelspacing
    return float(sy), float(sx)


def border(mask):
    mask = np.asarray(mask, dtype=bool)
    return mask & ~ndimage.binary_erosion(mask, structure=_CROSS, iterations=1, border_value=0)


def directed(a, b, voxelspacing=None):
    """sds(a, b): for every border pixel of ``a`` (row-major order) the distance to the nearest border pixel of ``b``"""
    a, b = np.asarray(a, dtype=bool), np.asarray(b, dtype=bool)
    if not a.any():
        raise RuntimeError("The first supplied array does not contain any binary object.")
    if not b.any():
        raise RuntimeError("The second supplied array does not contain any binary object.")
    dt = ndimage.distance_transform_edt(~border(b), sampling=_spacing(voxelspacing))
    return dt[border(a)]


def directed_brute(a, b, voxelspacing=None):
    """the same multiset by an all-pairs search"""
    a, b = np.asarray(a, dtype=bool), np.asarray(b, dtype=bool)
    if not a.any() or not b.any():
        raise RuntimeError("an array does not contain any binary object.")
    sy, sx = _spacing(voxelspacing)
    p, q = np.argwhere(border(a)).astype(np.float64), np.argwhere(border(b)).astype(np.float64)
    dy = (p[:, None, 0] - q[None, :, 0]) * sy
    dx = (p[:, None, 1] - q[None, :, 1]) * sx
    return np.sqrt(dy * dy + dx * dx).min(axis=1)


def hausdorff(a, b, voxelspacing=None, directed_fn=directed):
    return max(directed_fn(a, b, voxelspacing).max(), directed_fn(b, a, voxelspacing).max())


def mod_hausdorff(a, b, voxelspacing=None, percentile=95, directed_fn=directed):
    return max(np.percentile(directed_fn(a, b, voxelspacing), percentile),
               np.percentile(directed_fn(b, a, voxelspacing), percentile))


def average_surface(a, b, voxelspacing=None, directed_fn=directed):
    return (directed_fn(a, b, voxelspacing).mean() + directed_fn(b, a, voxelspacing).mean()) / 2.0


def surface_distances(pred, target, C, report_axis=None, voxelspacing=None, percentile=95.0):
    """class-coded [B,H,W] maps -> dict of [B, n_report] arrays: hd, mhd, asd (NaN where empty), empty (bool), n (the larger
    border-pixel count of the pair: the number of terms of the longer directed mean)"""
    pred, target = np.asarray(pred), np.asarray(target)
    report = list(range(C)) if report_axis is None else list(report_axis)
    B = pred.shape[0]
    out = {k: np.full((B, len(report)), np.nan) for k in ("hd", "mhd", "asd")}
    out["empty"] = np.zeros((B, len(report)), dtype=bool)
    out["n"] = np.zeros((B, len(report)), dtype=np.int64)
    for b in range(B):
        for r, c in enumerate(report):
            a, t = pred[b] == c, target[b] == c
            if not a.any() or not t.any():
                out["empty"][b, r] = True
                continue
            out["hd"][b, r] = hausdorff(a, t, voxelspacing)
            out["mhd"][b, r] = mod_hausdorff(a, t, voxelspacing, percentile)
            out["asd"][b, r] = average_surface(a, t, voxelspacing)
            out["n"][b, r] = max(int(border(a).sum()), int(border(t).sum()))
    return out


def meter(batches, C, report_axis, metername, voxelspacing=None):
    """``SurfaceMeter`` over (pred, target) batches: a batch in which any reported (slice, class) is empty is dropped (the
    reference's raise inside ``add``, ignored by its caller) -> (mean, std, skipped batches, rows)"""
    key = {"hausdorff": "hd", "mod_hausdorff": "mhd", "average_surface": "asd"}[metername]
    rows, skipped = [], 0
    for pred, target in batches:
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


# ---- seeded maps
def blob_maps(B, H, W, C, seed):
    """class-coded [B,H,W] map: arg-max of C smoothed noise fields; every class 0 .. C-1 is present in every sample (needs
    H * W >= C)"""
    assert H * W >= C
    rng = np.random.RandomState(seed)
    out = np.zeros((B, H, W), dtype=np.int64)
    for b in range(B):
        fields = np.stack([ndimage.gaussian_filter(rng.randn(H, W), sigma=max(0.6, min(H, W) / 8.0), mode="nearest")
                           for _ in range(C)])
        m = fields.argmax(0).reshape(-1)
        for _ in range(2 * C):  # stamp a pixel of every missing class (a stamp may remove another class's last pixel: repeat)
            missing = [c for c in range(C) if not (m == c).any()]
            if not missing:
                break
            for c in missing:
                m[(c * (H * W // C) + rng.randint(0, max(1, H * W // C))) % (H * W)] = c
        assert all((m == c).any() for c in range(C))
        out[b] = m.reshape(H, W)
    return out


def random_maps(B, H, W, C, seed):
    """per-pixel uniform random labels: nearly every pixel is a border pixel (the dense worst case)"""
    return np.random.RandomState(seed).randint(0, C, size=(B, H, W)).astype(np.int64)


def line_against_pixel(n, start=3):
    """target: one pixel at (0, 0); pred: n pixels of row 0 from column ``start`` -- every one a border pixel, at the distinct
    distances start .. start + n - 1; the converse directed set is the single value ``start``"""
    pred, target = np.zeros((2, start + n + 2), bool), np.zeros((2, start + n + 2), bool)
    pred[0, start:start + n], target[0, 0] = True, True
    return pred, target
