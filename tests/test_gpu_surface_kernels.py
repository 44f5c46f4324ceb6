"""``functional.surface_distances`` (csrc/surface.hip: exact separable distance transform, device-side maximum, radix-selected
percentile, ordered mean) against the float64 scipy oracle of tests/_surface_oracle.py.

Bars (eps = 2^-52, d_max = the pair's largest directed distance = its oracle ``hd``, n = the larger border-pixel count):
  hd     unit spacing: equal -- one correctly rounded float64 sqrt of an exact integer; with spacing 4 eps relative (two
         products, one sum possibly contracted to an FMA, one sqrt)
  mhd    16 eps d_max absolute (two such order statistics and the interpolation)
  asd    (n + 8) eps d_max absolute (worst case of a reordered sum of n non-negative terms)
  empty  equal; hd, mhd, asd are NaN exactly there
Every comparison prints its largest deviation in units of its bar before it asserts."""
import ctypes

import numpy as np
import pytest
import torch

from tests import _surface_oracle as O

pytestmark = pytest.mark.gpu

SPACINGS = [None, 2.0, (1.25, 0.7)]


def _run(pred, target, C, report=None, spacing=None, percentile=95.0):
    import spcl_amd  # noqa: F401
    from spcl_amd import functional as F_hip
    p, t = torch.from_numpy(np.ascontiguousarray(pred)).cuda(), torch.from_numpy(np.ascontiguousarray(target)).cuda()
    hd, mhd, asd, empty = F_hip.surface_distances(p, t, C, report, spacing, percentile)
    assert hd.dtype == mhd.dtype == asd.dtype == torch.float64 and empty.dtype == torch.uint8
    return hd.cpu().numpy(), mhd.cpu().numpy(), asd.cpu().numpy(), empty.cpu().numpy().astype(bool)


def _check(pred, target, C, report=None, spacing=None, percentile=95.0, what=""):
    want = O.surface_distances(pred, target, C, report, spacing, percentile)
    hd, mhd, asd, empty = _run(pred, target, C, report, spacing, percentile)
    assert hd.shape == want["hd"].shape
    assert np.array_equal(empty, want["empty"]), (what, empty, want["empty"])
    for v in (hd, mhd, asd):
        assert np.array_equal(np.isnan(v), want["empty"]), what
    ok = ~want["empty"]
    if not ok.any():
        return
    dmax, n = want["hd"][ok], want["n"][ok]
    unit = O._spacing(spacing) == (1.0, 1.0)
    e_hd = np.abs(hd[ok] - want["hd"][ok])
    e_mhd = np.abs(mhd[ok] - want["mhd"][ok])
    e_asd = np.abs(asd[ok] - want["asd"][ok])
    tiny = np.finfo(np.float64).tiny
    print(f"{what} spacing {spacing} q {percentile} report {report}: hd max rel err {float((e_hd / np.maximum(dmax, tiny)).max()):.3e}"
          f" (bar {'0' if unit else '4 eps'}), mhd {float((e_mhd / np.maximum(16 * O.EPS * dmax, tiny)).max()):.3f} bars, "
          f"asd {float((e_asd / np.maximum((n + 8) * O.EPS * dmax, tiny)).max()):.3f} bars, d_max {float(dmax.max()):.3f}, n {int(n.max())}")
    if unit:
        assert np.array_equal(hd[ok], want["hd"][ok]), (what, hd, want["hd"])
    else:
        assert (e_hd <= 4 * O.EPS * dmax).all(), (what, hd, want["hd"])
    assert (e_mhd <= 16 * O.EPS * dmax).all(), (what, mhd, want["mhd"])
    assert (e_asd <= (n + 8) * O.EPS * dmax).all(), (what, asd, want["asd"])


def _tiny_maps(B, H, W, seed):
    """two-class maps for the degenerate shapes: random bits, class 1 present in every sample of both maps"""
    rng = np.random.RandomState(seed)
    maps = []
    for _ in range(2):
        m = (rng.rand(B, H, W) < 0.4).astype(np.int64)
        for b in range(B):
            m[b].flat[rng.randint(H * W)] = 1
        maps.append(m)
    return maps


@pytest.mark.parametrize("shape", [(1, 1, 1), (2, 1, 7), (2, 5, 1), (3, 7, 9)])
def test_degenerate_shapes(shape):
    B, H, W = shape
    pred, target = _tiny_maps(B, H, W, seed=H * 100 + W)
    for spacing in SPACINGS:
        for q in (95.0, 50.0):
            _check(pred, target, 2, [1], spacing, q, what=f"tiny {shape}")
    if H * W >= 4:
        pred, target = O.blob_maps(B, H, W, 4, seed=11), O.blob_maps(B, H, W, 4, seed=12)
        for report in (None, [1, 2, 3], [2]):
            _check(pred, target, 4, report, (1.25, 0.7), 95.0, what=f"blobs {shape}")


@pytest.mark.parametrize("shape", [(2, 9, 70), (2, 65, 70), (1, 70, 130)])
def test_blobs_beyond_one_wave(shape):
    B, H, W = shape
    pred, target = O.blob_maps(B, H, W, 4, seed=21 + W), O.blob_maps(B, H, W, 4, seed=22 + W)
    for spacing in SPACINGS:
        for q in (95.0, 50.0):
            for report in (None, [1, 2, 3], [2]):
                _check(pred, target, 4, report, spacing, q, what=f"blobs {shape}")


def test_random_labels_dense_worst_case_and_same_bits_twice():
    pred, target = O.random_maps(2, 65, 70, 4, seed=31), O.random_maps(2, 65, 70, 4, seed=32)
    for spacing in SPACINGS:
        for q in (95.0, 50.0):
            _check(pred, target, 4, [1, 2, 3], spacing, q, what="random labels (2, 65, 70)")
    _check(pred, target, 4, None, None, 95.0, what="random labels (2, 65, 70)")
    _check(pred, target, 4, [2], (1.25, 0.7), 50.0, what="random labels (2, 65, 70)")
    for spacing in (None, (1.25, 0.7)):
        a, b = _run(pred, target, 4, [1, 2, 3], spacing), _run(pred, target, 4, [1, 2, 3], spacing)
        for x, y in zip(a, b):
            assert x.tobytes() == y.tobytes()


def test_workload_size_once_and_same_bits_twice():
    pred, target = O.blob_maps(2, 224, 224, 4, seed=41), O.blob_maps(2, 224, 224, 4, seed=42)
    _check(pred, target, 4, [1, 2, 3], None, 95.0, what="blobs (2, 224, 224)")
    a, b = _run(pred, target, 4, [1, 2, 3]), _run(pred, target, 4, [1, 2, 3])
    for x, y in zip(a, b):
        assert x.tobytes() == y.tobytes()


def test_objects_touching_every_edge_and_corner():
    H, W = 23, 70
    pred, target = np.zeros((2, H, W), np.int64), np.zeros((2, H, W), np.int64)
    pred[0, :3, :4] = 1         # the four corners
    pred[0, -2:, -5:] = 1
    pred[0, :2, -3:] = 2
    pred[0, -4:, :2] = 3
    target[0, 0, :] = 1         # whole edges
    target[0, :, -1] = 2
    target[0, -1, :30] = 3
    pred[1, :, 0] = 1
    pred[1, 5:9, -1] = 2
    pred[1, -1, 10:60] = 3
    target[1, 8:15, :3] = 1
    target[1, :, -2:] = 2
    target[1, 3:6, 20:66] = 3
    target[1, -1, -1] = 3
    for spacing in SPACINGS:
        _check(pred, target, 4, None, spacing, 95.0, what="edges and corners")
        _check(pred, target, 4, [1, 2, 3], spacing, 50.0, what="edges and corners")
    full = np.ones((1, 9, 70), np.int64)  # a full-image mask: the frame is its border
    dot = np.zeros((1, 9, 70), np.int64)
    dot[0, 4, 35] = 1
    _check(full, dot, 2, [1], None, 95.0, what="full image against a pixel")
    _check(dot, full, 2, [0, 1], (1.25, 0.7), 50.0, what="a pixel against the full image")


@pytest.mark.parametrize("shape", [(2, 9, 70), (2, 65, 70), (1, 70, 130), (1, 224, 224)])
def test_pred_equals_target_gives_zeros(shape):
    B, H, W = shape
    m = O.blob_maps(B, H, W, 4, seed=51)
    for spacing in (None, (1.25, 0.7)):
        hd, mhd, asd, empty = _run(m, m, 4, None, spacing)
        assert not empty.any() and not hd.any() and not mhd.any() and not asd.any()
        _check(m, m, 4, None, spacing, 95.0, what=f"pred = target {shape}")


@pytest.mark.parametrize("H,W", [(1, 7), (5, 1), (7, 9), (65, 70), (70, 130), (224, 224), (1024, 1024)])
def test_opposite_corners_largest_squared_distance(H, W):
    """one pixel each in opposite corners: the squared distance (H-1)^2 + (W-1)^2 is the largest the integer path sees"""
    pred, target = np.zeros((1, H, W), np.int64), np.zeros((1, H, W), np.int64)
    pred[0, 0, 0], target[0, H - 1, W - 1] = 1, 1
    hd, mhd, asd, empty = _run(pred, target, 2, [1])
    d = np.sqrt(np.float64((H - 1) ** 2 + (W - 1) ** 2))
    assert not empty.any() and hd[0, 0] == d and mhd[0, 0] == d and asd[0, 0] == d
    if H * W <= 224 * 224:
        for spacing in SPACINGS:
            _check(pred, target, 2, [1], spacing, 95.0, what=f"corners {H} x {W}")


def test_empty_classes_are_flagged_exactly_there():
    B, H, W = 3, 33, 70
    pred, target = O.blob_maps(B, H, W, 4, seed=61), O.blob_maps(B, H, W, 4, seed=62)
    pred[0][pred[0] == 2] = 0      # missing from pred
    target[1][target[1] == 3] = 0  # missing from target
    pred[2][pred[2] == 1] = 0      # missing from both
    target[2][target[2] == 1] = 0
    for spacing in (None, (1.25, 0.7)):
        for report in (None, [1, 2, 3], [2]):
            _check(pred, target, 4, report, spacing, 95.0, what="empty classes")
    want = O.surface_distances(pred, target, 4, [1, 2, 3])
    assert want["empty"].tolist() == [[False, True, False], [False, False, True], [True, False, False]]
    # the entries next to an empty one are those of maps in which nothing is missing from the OTHER samples
    full = O.surface_distances(O.blob_maps(B, H, W, 4, seed=61), O.blob_maps(B, H, W, 4, seed=62), 4, [1, 2, 3])
    hd = _run(pred, target, 4, [1, 2, 3])[0]
    assert hd[1, 0] == full["hd"][1, 0] and hd[0, 2] == full["hd"][0, 2] and hd[2, 2] == full["hd"][2, 2]


@pytest.mark.parametrize("n", [20, 21, 97])
def test_percentile_picks_the_same_two_ranks(n):
    """all directed distances distinct (a line of n pixels against one pixel: 3, 4, ..., n + 2 columns): an order statistic
    one rank off would miss by a whole column, 10^14 bars"""
    pred, target = O.line_against_pixel(n)
    pred, target = pred[None].astype(np.int64), target[None].astype(np.int64)
    for spacing in SPACINGS:
        for q in (95.0, 50.0, 0.0, 100.0, 37.3):
            _check(pred, target, 2, [1], spacing, q, what=f"line of {n}")
    hd, mhd, asd, _ = _run(pred, target, 2, [1], None, 95.0)
    want = np.percentile(np.arange(3.0, 3.0 + n), 95.0)
    assert abs(mhd[0, 0] - want) <= 16 * O.EPS * (n + 2) and hd[0, 0] == n + 2.0


def test_argument_validation_launches_nothing():
    import spcl_amd  # noqa: F401
    from spcl_amd import functional as F_hip
    from spcl_amd import native
    L = native.lib()
    assert L.spcl_surface_workspace_bytes(2, 1025, 8, 3) == 0 and L.spcl_surface_workspace_bytes(2, 8, 8, 65) == 0
    assert L.spcl_surface_workspace_bytes(2, 1024, 1024, 64) > 0

    def rc(H, W, C, report):
        # null data pointers: a call that got past its argument checks would say "null pointer", not launch
        arr = (ctypes.c_int * len(report))(*report)
        return L.spcl_surface_distances(None, None, 1, H, W, C, arr, len(report), 1.0, 1.0, 95.0, None, None, None, None, None,
                                        0, None), L.spcl_last_error().decode()

    code, msg = rc(1025, 8, 4, [1])
    assert code == -1 and "1024" in msg
    code, msg = rc(8, 8, 80, list(range(65)))
    assert code == -1 and "reported classes" in msg
    code, msg = rc(8, 8, 4, [1, 4])
    assert code == -1 and "class 4" in msg
    m = torch.zeros(1, 8, 8, dtype=torch.int64, device="cuda")
    with pytest.raises(RuntimeError, match="class 4"):
        F_hip.surface_distances(m, m, 4, [1, 4])
    with pytest.raises(RuntimeError, match="1024"):
        F_hip.surface_distances(torch.zeros(1, 1025, 2, dtype=torch.int64, device="cuda"),
                                torch.zeros(1, 1025, 2, dtype=torch.int64, device="cuda"), 2)
    with pytest.raises(RuntimeError, match="reported classes"):
        F_hip.surface_distances(m, m, 80, list(range(65)))
