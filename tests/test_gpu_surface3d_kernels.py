"""``functional.surface_distances_3d`` (csrc/surface.hip: slice-wise column scan with the 6-neighbour border test, the depth
pass along z, row minima over squared-distance rows, device-side maximum, radix-selected percentile, ordered mean) against the
float64 scipy oracle of tests/_surface3d_oracle.py.

Bars, those of tests/test_gpu_surface_kernels.py (eps = 2^-52, d_max = the pair's largest directed distance = its oracle
``hd``, n = the larger border-voxel count):
  hd     unit spacing: equal -- one correctly rounded float64 sqrt of an exact integer; with spacing 4 eps relative
  mhd    16 eps d_max absolute (two order statistics and the interpolation)
  asd    (n + 8) eps d_max absolute (worst case of a reordered sum of n non-negative terms)
  empty  equal; hd, mhd, asd are NaN exactly there
Every comparison prints its largest deviation in units of its bar before it asserts."""
import numpy as np
import pytest
import torch

from tests import _surface3d_oracle as O
from tests import _surface_oracle as O2

pytestmark = pytest.mark.gpu

SPACINGS = [None, O.ANISO]


def _run(pred, target, C, report=None, spacing=None, percentile=95.0):
    import spcl_amd  # noqa: F401
    from spcl_amd import functional as F_hip
    p, t = torch.from_numpy(np.ascontiguousarray(pred)).cuda(), torch.from_numpy(np.ascontiguousarray(target)).cuda()
    hd, mhd, asd, empty = F_hip.surface_distances_3d(p, t, C, report, spacing, percentile)
    V = 1 if pred.ndim == 3 else pred.shape[0]
    R = C if report is None else len(report)
    assert hd.shape == mhd.shape == asd.shape == empty.shape == (V, R)
    assert hd.dtype == mhd.dtype == asd.dtype == torch.float64 and empty.dtype == torch.uint8
    return hd.cpu().numpy(), mhd.cpu().numpy(), asd.cpu().numpy(), empty.cpu().numpy().astype(bool)


def _check(pred, target, C, report=None, spacing=None, percentile=95.0, what=""):
    want = O.surface_distances(pred, target, C, report, spacing, percentile)
    hd, mhd, asd, empty = got = _run(pred, target, C, report, spacing, percentile)
    assert hd.shape == want["hd"].shape
    assert np.array_equal(empty, want["empty"]), (what, empty, want["empty"])
    for v in (hd, mhd, asd):
        assert np.array_equal(np.isnan(v), want["empty"]), what
    ok = ~want["empty"]
    if not ok.any():
        return got
    dmax, n = want["hd"][ok], want["n"][ok]
    unit = O._spacing(spacing) == (1.0, 1.0, 1.0)
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
    return got


def _maps(shape, seed):
    V, D, H, W = shape
    if D * H * W < 4:
        return O.tiny_volumes(V, D, H, W, seed) + [2, [1]]
    return [O.blob_volumes(V, D, H, W, 4, seed), O.blob_volumes(V, D, H, W, 4, seed + 1), 4, [1, 2, 3]]


@pytest.mark.parametrize("spacing", SPACINGS)
@pytest.mark.parametrize("shape", [(1, 1, 1, 1), (1, 1, 5, 7), (1, 2, 1, 1), (2, 3, 7, 9), (1, 5, 9, 70), (1, 4, 65, 70),
                                   (1, 9, 20, 24)])
def test_shapes_against_the_oracle(shape, spacing):
    V, D, H, W = shape
    pred, target, C, report = _maps(shape, seed=D * 10000 + H * 100 + W)
    got = _check(pred, target, C, report, spacing, 95.0, what=f"{shape}")
    _check(pred, target, C, report, spacing, 50.0, what=f"{shape}")
    if C == 4:
        _check(pred, target, C, None, spacing, 95.0, what=f"{shape}")
        _check(pred, target, C, [2], spacing, 37.3, what=f"{shape}")
    if V > 1:  # every volume's row is the single-volume call's, bit for bit
        for v in range(V):
            one = _run(pred[v], target[v], C, report, spacing, 95.0)
            for x, y in zip(got, one):
                assert x[v].tobytes() == y[0].tobytes(), (shape, v)


@pytest.mark.parametrize("spacing", SPACINGS)
def test_one_slice_volume_is_not_the_slice_wise_call(spacing):
    """a 3 x 4 block against one pixel inside it: in the volume call every voxel of the block is a border voxel (the pixel
    lies ON the block's border, distance 0), slice-wise the two interior pixels are not (distance 1 from the pixel)"""
    import spcl_amd  # noqa: F401
    from spcl_amd import functional as F_hip
    pred, target = np.zeros((1, 1, 5, 7), np.int64), np.zeros((1, 1, 5, 7), np.int64)
    pred[0, 0, 1:4, 1:5], target[0, 0, 2, 2] = 1, 1
    hd3, mhd3, asd3, _ = _check(pred, target, 2, [1], spacing, 95.0, what="block against a pixel inside it")
    flat = None if spacing is None else spacing[1:]
    p, t = torch.from_numpy(pred[0]).cuda(), torch.from_numpy(target[0]).cuda()
    hd2, mhd2, asd2, _ = (x.cpu().numpy() for x in F_hip.surface_distances(p, t, 2, [1], flat, 95.0))
    want2 = O2.surface_distances(pred[0], target[0], 2, [1], flat, 95.0)
    assert abs(asd2[0, 0] - want2["asd"][0, 0]) <= (want2["n"][0, 0] + 8) * O.EPS * want2["hd"][0, 0]
    assert hd3[0, 0] == hd2[0, 0]  # (the farthest corner of the block is a border pixel either way)
    assert asd3[0, 0] < asd2[0, 0] and abs(asd3[0, 0] - asd2[0, 0]) > 0.1
    # and on blobs: wherever the oracles of the two definitions differ, so do the two calls
    bp, bt = O.blob_volumes(1, 1, 5, 7, 2, seed=507), O.blob_volumes(1, 1, 5, 7, 2, seed=508)
    w3, w2 = O.surface_distances(bp, bt, 2, None, spacing), O2.surface_distances(bp[0], bt[0], 2, None, flat)
    g3 = _check(bp, bt, 2, None, spacing, 95.0, what="one-slice blobs")
    g2 = [x.cpu().numpy() for x in F_hip.surface_distances(torch.from_numpy(bp[0]).cuda(), torch.from_numpy(bt[0]).cuda(), 2, None,
                                                           flat, 95.0)]
    differs = np.abs(w3["asd"] - w2["asd"]) > 1e-9
    assert np.array_equal(np.abs(g3[2] - g2[2]) > 1e-9, differs)


def test_random_labels_dense_worst_case_and_same_bits_twice():
    pred, target = O.random_volumes(1, 6, 33, 70, 4, seed=31), O.random_volumes(1, 6, 33, 70, 4, seed=32)
    for spacing in SPACINGS:
        for q in (95.0, 50.0):
            _check(pred, target, 4, [1, 2, 3], spacing, q, what="random labels (1, 6, 33, 70)")
        a, b = _run(pred, target, 4, [1, 2, 3], spacing), _run(pred, target, 4, [1, 2, 3], spacing)
        for x, y in zip(a, b):
            assert x.tobytes() == y.tobytes()


def test_workload_size_once_and_same_bits_twice():
    pred, target = O.blob_volumes(1, 10, 224, 224, 4, seed=41), O.blob_volumes(1, 10, 224, 224, 4, seed=42)
    for spacing in SPACINGS:
        _check(pred, target, 4, [1, 2, 3], spacing, 95.0, what="blobs (1, 10, 224, 224)")
        a, b = _run(pred, target, 4, [1, 2, 3], spacing), _run(pred, target, 4, [1, 2, 3], spacing)
        for x, y in zip(a, b):
            assert x.tobytes() == y.tobytes()


@pytest.mark.parametrize("shape", [(2, 3, 7, 9), (1, 5, 9, 70), (1, 4, 65, 70)])
def test_pred_equals_target_gives_zeros(shape):
    m = O.blob_volumes(*shape, 4, seed=51)
    for spacing in SPACINGS:
        hd, mhd, asd, empty = _run(m, m, 4, None, spacing)
        assert not empty.any() and not hd.any() and not mhd.any() and not asd.any()


@pytest.mark.parametrize("shape", [(7, 9, 11), (3, 224, 224)])
def test_opposite_corners(shape):
    """one voxel each in opposite corners: every value is sqrt((D-1)^2 + (H-1)^2 + (W-1)^2), one correctly rounded sqrt"""
    D, H, W = shape
    pred, target = np.zeros((1, D, H, W), np.int64), np.zeros((1, D, H, W), np.int64)
    pred[0, 0, 0, 0], target[0, D - 1, H - 1, W - 1] = 1, 1
    hd, mhd, asd, empty = _run(pred, target, 2, [1])
    d = np.sqrt(np.float64((D - 1) ** 2 + (H - 1) ** 2 + (W - 1) ** 2))
    assert not empty.any() and hd[0, 0] == d and mhd[0, 0] == d and asd[0, 0] == d
    _check(pred, target, 2, [1], O.ANISO, 95.0, what=f"corners {shape}")
    _check(target, pred, 2, [0, 1], None, 95.0, what=f"corners {shape}, background too")


def test_object_touching_all_six_faces():
    D, H, W = 5, 23, 70
    pred, target = np.zeros((1, D, H, W), np.int64), np.zeros((1, D, H, W), np.int64)
    pred[0, :, 10:13, 30:40] = 1  # a bar through every slice: the faces z = 0 and z = D - 1
    pred[0, 2, :, 33] = 1         # y = 0 and y = H - 1
    pred[0, 2, 11, :] = 1         # x = 0 and x = W - 1
    pred[0, 0, 0, 0] = 2          # corners and edges
    pred[0, -1, -1, -1] = 2
    pred[0, :, 0, -1] = 3
    target[0] = 1                 # the full volume: its border is the shell
    target[0, 1:3, 5:9, 50:60] = 2
    target[0, -1, :, 0] = 3
    for ax, size in enumerate((D, H, W)):  # class 1 of pred reaches both ends of every axis
        idx = np.argwhere(pred[0] == 1)[:, ax]
        assert idx.min() == 0 and idx.max() == size - 1
    for spacing in SPACINGS:
        _check(pred, target, 4, [1, 2, 3], spacing, 95.0, what="six faces")
        _check(target, pred, 4, [1, 2, 3], spacing, 50.0, what="six faces, swapped")


def test_absent_classes_are_flagged_exactly_there():
    V, D, H, W = 3, 4, 17, 70
    full_p, full_t = O.blob_volumes(V, D, H, W, 4, seed=61), O.blob_volumes(V, D, H, W, 4, seed=62)
    pred, target = full_p.copy(), full_t.copy()
    pred[0][pred[0] == 2] = 0      # missing from the whole volume of pred only
    target[1][target[1] == 3] = 0  # of target only
    pred[2][pred[2] == 1] = 0      # of both
    target[2][target[2] == 1] = 0
    pred[1, 0][pred[1, 0] == 2] = 0  # missing from one SLICE only: not an empty class of the volume
    for spacing in SPACINGS:
        for report in (None, [1, 2, 3], [2]):
            _check(pred, target, 4, report, spacing, 95.0, what="absent classes")
    want = O.surface_distances(pred, target, 4, [1, 2, 3])
    assert want["empty"].tolist() == [[False, True, False], [False, False, True], [True, False, False]]
    # the classes next to an absent one are unaffected wherever the edit left both of their masks alone
    full = O.surface_distances(full_p, full_t, 4, [1, 2, 3])
    hd = _run(pred, target, 4, [1, 2, 3])[0]
    assert hd[0, 2] == full["hd"][0, 2] and hd[1, 0] == full["hd"][1, 0] and hd[2, 2] == full["hd"][2, 2]


@pytest.mark.parametrize("n", [20, 21, 97])
def test_percentile_picks_the_same_two_ranks(n):
    """all directed distances distinct (a line of n voxels along z against one voxel: 3, 4, ..., n + 2 slices): an order
    statistic one rank off would miss by a whole slice, 10^14 bars"""
    pred, target = O.line_against_voxel(n)
    pred, target = pred[None].astype(np.int64), target[None].astype(np.int64)
    for spacing in SPACINGS:
        for q in (95.0, 50.0, 0.0, 100.0, 37.3):
            _check(pred, target, 2, [1], spacing, q, what=f"line of {n}")
    hd, mhd, asd, _ = _run(pred, target, 2, [1], None, 95.0)
    want = np.percentile(np.arange(3.0, 3.0 + n), 95.0)
    assert abs(mhd[0, 0] - want) <= 16 * O.EPS * (n + 2) and hd[0, 0] == n + 2.0
    mhd5 = _run(pred, target, 2, [1], O.ANISO, 95.0)[1]
    assert abs(mhd5[0, 0] - 5.0 * want) <= 16 * O.EPS * 5.0 * (n + 2)


def test_argument_validation_raises_and_workspace_is_cached_per_shape():
    import spcl_amd  # noqa: F401
    from spcl_amd import functional as F_hip
    m = torch.zeros(2, 8, 8, dtype=torch.int64, device="cuda")
    with pytest.raises(RuntimeError, match="class 4"):
        F_hip.surface_distances_3d(m, m, 4, [1, 4])
    with pytest.raises(RuntimeError, match="1024"):
        big = torch.zeros(1025, 2, 2, dtype=torch.int64, device="cuda")
        F_hip.surface_distances_3d(big, big, 2)
    with pytest.raises(RuntimeError, match="spacing"):
        F_hip.surface_distances_3d(m, m, 2, None, (0.0, 1.0, 1.0))
    with pytest.raises(RuntimeError, match="percentile"):
        F_hip.surface_distances_3d(m, m, 2, None, None, 101.0)
    F_hip.surface_distances_3d(m, m, 2, [1])
    key = (m.device, 1, 2, 8, 8, 1)
    ws = F_hip._SURFACE3D_WS[key]
    F_hip.surface_distances_3d(m, m, 2, [0], 2.0)
    assert F_hip._SURFACE3D_WS[key] is ws
    hd, _, _, empty = F_hip.surface_distances_3d(m.unsqueeze(0), m.unsqueeze(0), 2, [0, 1], 2.0)
    assert empty.cpu().tolist() == [[0, 1]] and hd[0, 0].item() == 0.0
