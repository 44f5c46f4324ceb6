"""``functional.largest_components`` / ``spcl_largest_component`` against the scipy restatement of tests/_lcc_oracle.py.  Every
comparison is EXACT equality of the processed map, ``kept_size`` and ``n_components``: the values are integers, no tolerance
applies.  The kernel tiles a slice 32 x 64 in LDS and processes 2048 consecutive voxels per workgroup afterwards: the shapes
below cross those borders (33 x 65 holds two tiles in each direction), stay inside one tile, or are degenerate."""
import ctypes

import numpy as np
import pytest
import torch

from tests import _lcc_oracle as O

pytestmark = pytest.mark.gpu


def _run(labels, C, classes=None, volumetric=True):
    import spcl_amd  # noqa: F401
    from spcl_amd import functional as F_hip
    t = torch.from_numpy(np.ascontiguousarray(labels)).cuda()
    extras = []
    got = F_hip.largest_components(t, C, classes=classes, volumetric=volumetric, out=extras)
    assert got.dtype == torch.int64 and got.shape == t.shape and got.is_cuda
    kept, ncomp = extras
    assert kept.dtype == torch.int64 and ncomp.dtype == torch.int32 and kept.is_cuda and ncomp.is_cuda
    assert np.array_equal(t.cpu().numpy(), labels)  # the input is not modified
    return got.cpu().numpy(), kept.cpu().numpy(), ncomp.cpu().numpy()


def _check(labels, C, classes=None, volumetric=True):
    want = O.largest_components(labels, C, classes, volumetric)
    got = _run(labels, C, classes, volumetric)
    for name, g, w in zip(("processed", "kept_size", "n_components"), got, want):
        assert g.shape == w.shape, (name, g.shape, w.shape)
        assert np.array_equal(g, w), (name, int((g != w).sum()), g.ravel()[:16], w.ravel()[:16])
    return want


def _map(rows):
    return np.array([[int(ch) for ch in r] for r in rows], np.int64)[None, None]


def test_hand_made_diagonal_contact():
    m = _map(["1100000",
              "1100000",
              "0011100",
              "0011100",
              "0000022"])
    out, kept, ncomp = _check(m, 3)
    assert ncomp.tolist() == [[2, 1]] and kept.tolist() == [[6, 2]] and out[0, 0, 0, 0] == 0 and out[0, 0, 4, 6] == 2


def test_hand_made_tie_goes_to_the_first_in_raster_order():
    m = _map(["0000110",
              "0000110",
              "1100000",
              "1100000",
              "0000000"])
    out, kept, ncomp = _check(m, 2)
    assert ncomp.tolist() == [[2]] and kept.tolist() == [[4]] and out[0, 0, 0, 4] == 1 and out[0, 0, 2, 0] == 0


def test_hand_made_class_listed_but_absent():
    m = _map(["1100000",
              "0000000",
              "0000300",
              "0000300",
              "0000000"])
    out, kept, ncomp = _check(m, 4)
    assert kept.tolist() == [[2, 0, 2]] and ncomp.tolist() == [[1, 0, 1]] and np.array_equal(out, m)


def test_serpentine_across_every_tile_border():
    """33 x 65 with 32 x 64 tiles: two tiles in each direction; the long snake runs through all four, every row of it crosses
    the vertical tile border, and its union chain is hundreds of links long"""
    m = O.serpentine(33, 65)
    out, kept, ncomp = _check(m, 2, classes=[1])
    assert ncomp.tolist() == [[2]] and kept[0, 0] == (out != 0).sum() > 700


def test_serpentine_along_columns():
    """the same snake turned by 90 degrees: inside a tile every voxel is a run of its own and every join is a vertical union"""
    m = np.ascontiguousarray(O.serpentine(65, 33).transpose(0, 1, 3, 2))
    assert m.shape == (1, 1, 33, 65)
    _, kept, ncomp = _check(m, 2, classes=[1])
    assert ncomp.tolist() == [[2]]


def test_bridge_along_z_only():
    v = np.zeros((1, 4, 12, 20), np.int64)
    v[0, 1, 1:5, 2:8] = 2     # 24 voxels
    v[0, 2, 4:10, 7:15] = 2   # 48 voxels; (1, 4, 7) and (2, 4, 7) are the one pair in contact
    v[0, 0, 9:12, 0:9] = 2    # 27 voxels, on their own
    v[0, 3, 0:2, 16:20] = 1
    assert ((v[0, 1] == 2) & (v[0, 2] == 2)).sum() == 1
    out, kept, ncomp = _check(v, 3)
    assert kept.tolist() == [[8, 72]] and ncomp.tolist() == [[1, 2]] and (out[0, 0] == 0).all()
    # the same tensor as four slices: each decides on its own
    out, kept, ncomp = _check(v[0], 3, volumetric=False)
    assert kept[:, 1].tolist() == [27, 24, 48, 0] and np.array_equal(out, v[0])


def test_random_labels_two_volumes():
    """uniform labels per voxel: thousands of components of 1 to ~10 voxels, many equal sizes, W no multiple of 64"""
    m = O.random_labels((2, 6, 40, 72), 4, seed=5)
    _, kept, ncomp = _check(m, 4)
    assert (ncomp > 1000).all() and (kept < 200).all()
    _check(m[0], 4, volumetric=False)  # six slices, 4-neighbour


@pytest.mark.parametrize("shape", [(1, 1, 9, 33), (1, 3, 1, 1), (1, 1, 1, 64), (1, 5, 7, 1), (2, 2, 33, 1)])
def test_edge_shapes(shape):
    _check(O.random_labels(shape, 3, seed=sum(shape)), 3)
    ones = np.ones(shape, np.int64)
    out, kept, ncomp = _check(ones, 3)  # all voxels one class
    n = int(np.prod(shape[1:]))
    assert kept.tolist() == [[n, 0]] * shape[0] and ncomp.tolist() == [[1, 0]] * shape[0] and np.array_equal(out, ones)
    out, kept, ncomp = _check(np.zeros(shape, np.int64), 3)  # all background
    assert not kept.any() and not ncomp.any() and not out.any()


def test_partial_class_list_leaves_the_other_labels_alone():
    m = O.random_labels((1, 3, 20, 70), 4, seed=9)
    m[0, 0, 0, :5] = [7, -1, 4, 7, 7]  # values outside [0, C) are not listed either
    out, kept, ncomp = _check(m, 4, classes=[2])
    assert kept.shape == (1, 1)
    for other in (1, 3, 7, -1, 4):
        assert np.array_equal(out == other, m == other)
    assert (out == 2).sum() == kept[0, 0] < (m == 2).sum()
    _check(m, 4, classes=[3, 1])  # listed out of order: outputs follow the list


@pytest.fixture(scope="module")
def full_size():
    m = O.smooth_blobs((1, 10, 224, 224), 4, seed=11)
    return m, O.largest_components(m, 4)


def test_full_size_blobs_with_islands(full_size):
    m, want = full_size
    assert all((m == c).sum() > 5000 for c in (1, 2, 3)) and (want[2] > 50).all()
    got = _run(m, 4)
    for g, w in zip(got, want):
        assert np.array_equal(g, w)


def test_same_bits_on_every_run_and_for_a_permuted_input(full_size):
    m, want = full_size
    first = _run(m, 4)
    second = _run(m, 4)
    assert all(np.array_equal(a, b) for a, b in zip(first, second))
    import spcl_amd  # noqa: F401
    from spcl_amd import functional as F_hip
    small = O.random_labels((6, 40, 72), 4, seed=6)
    base = torch.from_numpy(np.ascontiguousarray(small.transpose(2, 0, 1))).cuda()
    view = base.permute(1, 2, 0)  # the same [6, 40, 72] values, not contiguous
    assert not view.is_contiguous() and np.array_equal(view.cpu().numpy(), small)
    a = F_hip.largest_components(view, 4)
    b = F_hip.largest_components(view.contiguous(), 4)
    assert torch.equal(a, b) and np.array_equal(a.cpu().numpy(), O.largest_components(small, 4)[0])
    assert np.array_equal(view.cpu().numpy(), small)


def test_call_is_capturable():
    """no readback, no allocation inside the call: it records into a hipGraph (the first call of the shape allocates the cached
    workspace and runs eagerly)"""
    import spcl_amd  # noqa: F401
    from spcl_amd import functional as F_hip
    m = O.random_labels((1, 4, 33, 65), 4, seed=8)
    t = torch.from_numpy(m).cuda()
    want = F_hip.largest_components(t, 4)
    torch.cuda.synchronize()
    g, side = torch.cuda.CUDAGraph(), torch.cuda.Stream()
    with torch.cuda.graph(g, stream=side):
        got = F_hip.largest_components(t, 4)
    g.replay()
    torch.cuda.synchronize()
    assert torch.equal(got, want) and np.array_equal(want.cpu().numpy(), O.largest_components(m, 4)[0])


def test_refusals():
    import spcl_amd  # noqa: F401
    from spcl_amd import functional as F_hip
    from spcl_amd import native as _n
    t = torch.zeros(2, 8, 8, dtype=torch.int64, device="cuda")
    with pytest.raises(TypeError, match="class-coded integer"):
        F_hip.largest_components(t.float(), 4)
    for bad in ([0], [4], [1, 4], [1, 2, 1], []):
        with pytest.raises(ValueError, match="classes"):
            F_hip.largest_components(t, 4, classes=bad)
    with pytest.raises(ValueError, match="classes"):
        F_hip.largest_components(t, 1)
    with pytest.raises(RuntimeError, match="MI355X"):
        F_hip.largest_components(t.cpu(), 4)
    # through the C ABI: `out` aliasing `labels` (wholly, or partly: mismatched starts) is refused before any launch
    nbytes = _n.call("spcl_largest_component_workspace_bytes", 1, 2, 8, 8, 1)
    ws = torch.empty(nbytes, dtype=torch.uint8, device="cuda")
    kept = torch.zeros(1, 1, dtype=torch.int64, device="cuda")
    ncomp = torch.zeros(1, 1, dtype=torch.int32, device="cuda")
    big = torch.ones(3, 8, 8, dtype=torch.int64, device="cuda")
    cls = (ctypes.c_int * 1)(1)
    for labels, out in ((big[:2], big[:2]), (big[:2], big[1:]), (big[1:], big[:2])):
        with pytest.raises(RuntimeError, match="alias"):
            _n.call("spcl_largest_component", _n.ptr(labels), 1, 2, 8, 8, 4, cls, 1, _n.ptr(out), _n.ptr(kept), _n.ptr(ncomp),
                    _n.ptr(ws), nbytes, _n.stream())
    torch.cuda.synchronize()
    assert bool((big == 1).all())  # nothing was written
