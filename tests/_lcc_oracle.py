"""Float-free restatement of the largest-connected-component step (``functional.largest_components`` /
``spcl_largest_component``) with ``scipy.ndimage.label``: default cross-shaped structure (4-connectivity in a slice,
6-connectivity in a volume), applied per volume and class; ``bincount`` of the component numbers, FIRST ``argmax`` -- scipy
numbers components in raster order of their first voxel, so equal sizes go to the component that starts first.  Everything is
integers.  Also the seeded inputs the GPU tests and the timing script share."""
import numpy as np
from scipy import ndimage


def largest_components(labels, num_classes, classes=None, volumetric=True):
    """labels: integer [D,H,W] / [V,D,H,W] (``volumetric=False``: [B,H,W] as B slices) -> (processed int64 in the shape of
    ``labels``, kept_size int64 [V, n_classes], n_components int32 [V, n_classes])"""
    lab = np.asarray(labels).astype(np.int64)
    shape = lab.shape
    if lab.ndim == 3:
        lab = lab[None] if volumetric else lab[:, None]
    assert lab.ndim == 4, shape
    cls = list(range(1, num_classes)) if classes is None else [int(c) for c in classes]
    out = lab.copy()
    kept = np.zeros((lab.shape[0], len(cls)), np.int64)
    ncomp = np.zeros((lab.shape[0], len(cls)), np.int32)
    for v in range(lab.shape[0]):
        for i, c in enumerate(cls):
            comp, n = ndimage.label(lab[v] == c)  # (default structure: faces only)
            ncomp[v, i] = n
            if n == 0:
                continue
            sizes = np.bincount(comp.ravel())
            sizes[0] = 0  # (0 is "not this class")
            win = int(np.argmax(sizes))
            kept[v, i] = sizes[win]
            out[v][(comp != 0) & (comp != win)] = 0
    return out.reshape(shape), kept, ncomp


def removed_fraction(before, after):
    """fraction of the foreground voxels of ``before`` that ``after`` no longer holds (0 where there are none)"""
    b, a = int((np.asarray(before) != 0).sum()), int((np.asarray(after) != 0).sum())
    return (b - a) / max(b, 1)


# ---- inputs
def serpentine(H, W, label=1):
    """[1,1,H,W]: a one-voxel-wide snake through every even row (full rows joined alternately at the right and the left end by
    one voxel of the odd row between them) -- ONE component -- and, cut off from it, a shorter snake over the first rows"""
    m = np.zeros((H, W), np.int64)
    cut = (H // 3) | 1  # an odd row left empty: the short snake ends above it, the long one starts below it
    for y in range(0, H, 2):
        m[y] = label
    for k, y in enumerate(range(1, H - 1, 2)):
        if y != cut:
            m[y, W - 1 if k % 2 == 0 else 0] = label
    return m[None, None]


def random_labels(shape, C, seed):
    return np.random.default_rng(seed).integers(0, C, size=shape).astype(np.int64)


def smooth_blobs(shape, C, seed, islands=0.002):
    """[V,D,H,W]: thresholded low-pass noise (a few large blobs per class) with single-voxel islands sprinkled over it"""
    rng = np.random.default_rng(seed)
    V, D, H, W = shape
    field = ndimage.gaussian_filter(rng.standard_normal(shape), sigma=(0, 1.5, 12, 12))
    field = field / field.std()
    lab = np.zeros(shape, np.int64)
    for c, t in zip(range(1, C), np.linspace(0.6, 1.6, C - 1)):
        lab[field > t] = c
        lab[field < -t] = C - c
    spots = rng.random(shape) < islands
    lab[spots] = rng.integers(1, C, size=int(spots.sum()))
    return lab
