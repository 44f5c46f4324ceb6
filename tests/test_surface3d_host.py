"""CPU-only: the per-scan surface-distance oracle (tests/_surface3d_oracle.py) against the all-pairs formulation, bit for bit;
the two native entry points of the volume path (binding table, argument checks that launch nothing); the host side of
``VolumeSurfaceMeter``; ``InferenceEpocher``'s default meter set."""
import ctypes
import math

import numpy as np
import pytest
import torch

from tests import _surface3d_oracle as O

SHAPES = [(1, 5, 7), (2, 1, 1), (3, 7, 9), (5, 9, 70)]


@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("spacing", [None, O.ANISO])
def test_oracle_equals_all_pairs_bit_for_bit(shape, spacing):
    rng = np.random.RandomState(shape[0] * 1009 + shape[1] * 131 + shape[2])
    for density in (0.05, 0.3, 0.6, 0.95):
        a, b = rng.rand(*shape) < density, rng.rand(*shape) < density
        a.flat[rng.randint(a.size)] = True  # (an empty mask raises: tested below)
        b.flat[rng.randint(b.size)] = True
        for x, y in ((a, b), (b, a)):
            got, want = O.directed(x, y, spacing), O.directed_brute(x, y, spacing)
            assert got.shape == want.shape and got.tobytes() == want.tobytes(), float(np.abs(got - want).max())
        assert O.hausdorff(a, b, spacing, directed_fn=O.directed) == O.hausdorff(a, b, spacing, directed_fn=O.directed_brute)
        o = O.surface_distances(a[None].astype(np.int64), b[None].astype(np.int64), 2, [1], spacing)
        assert o["hd"][0, 0] == O.hausdorff(a, b, spacing, directed_fn=O.directed_brute)
        assert o["mhd"][0, 0] == O.mod_hausdorff(a, b, spacing, directed_fn=O.directed_brute)
        assert o["asd"][0, 0] == O.average_surface(a, b, spacing, directed_fn=O.directed_brute)


def test_border_is_the_six_neighbour_one():
    full = np.ones((4, 5, 6), bool)
    shell = full.copy()
    shell[1:-1, 1:-1, 1:-1] = False
    assert np.array_equal(O.border(full), shell)
    one_slice = np.zeros((1, 5, 7), bool)
    one_slice[0, 1:4, 1:5] = True
    assert np.array_equal(O.border(one_slice), one_slice)  # no neighbour in z: every voxel of the object
    from tests import _surface_oracle as O2
    assert int(O2.border(one_slice[0]).sum()) == one_slice.sum() - 2  # the slice-wise border leaves the interior out
    a, e = np.ones((2, 3, 3), bool), np.zeros((2, 3, 3), bool)
    for x, y in ((a, e), (e, a), (e, e)):
        with pytest.raises(RuntimeError):
            O.directed(x, y)


def test_generators_put_every_class_into_every_volume():
    for m in (O.blob_volumes(2, 3, 7, 9, 4, seed=1), O.blob_volumes(1, 1, 5, 7, 4, seed=2), O.random_volumes(1, 6, 33, 70, 4, seed=3)):
        assert m.dtype == np.int64 and all((m[v] == c).any() for v in range(m.shape[0]) for c in range(4))
    for m in O.tiny_volumes(1, 2, 1, 1, seed=4):
        assert (m == 1).any()
    p, t = O.line_against_voxel(20)
    assert np.array_equal(np.sort(O.directed(p, t)), np.arange(3.0, 23.0)) and np.array_equal(O.directed(t, p), [3.0])


# ---- native entry points
def test_native_table_lists_the_volume_entry_points():
    import spcl_amd  # noqa: F401
    from spcl_amd import native
    assert native.ABI_VERSION >= 18
    for name in ("spcl_surface_3d_workspace_bytes", "spcl_surface_distances_3d"):
        assert name in native._SIGNATURES and hasattr(native.lib(), name)
    assert native._SIGNATURES["spcl_surface_3d_workspace_bytes"][0] is ctypes.c_size_t
    assert len(native._SIGNATURES["spcl_surface_distances_3d"][1]) == 20


def test_argument_checks_report_minus_one_and_launch_nothing():
    import spcl_amd  # noqa: F401
    from spcl_amd import native
    L = native.lib()
    assert L.spcl_surface_3d_workspace_bytes(1, 1025, 8, 8, 3) == 0 and L.spcl_surface_3d_workspace_bytes(1, 8, 8, 8, 65) == 0
    assert L.spcl_surface_3d_workspace_bytes(1, 2048, 1024, 1024, 1) == 0
    n = 10 * 224 * 224
    assert L.spcl_surface_3d_workspace_bytes(1, 10, 224, 224, 3) >= 6 * n * (2 + 8 + 8)

    def rc(D, H, W, C, report, spacing=(1.0, 1.0, 1.0)):
        # null data pointers: a call that got past its argument checks would say "null pointer", not launch
        arr = (ctypes.c_int * len(report))(*report)
        code = L.spcl_surface_distances_3d(None, None, 1, D, H, W, C, arr, len(report), *spacing, 95.0, None, None, None, None,
                                           None, 0, None)
        return code, L.spcl_last_error().decode()

    code, msg = rc(1025, 8, 8, 4, [1])
    assert code == -1 and "1024" in msg
    code, msg = rc(2048, 1024, 1024, 4, [1])  # D H W = 2^31
    assert code == -1 and ("1024" in msg or "2^31" in msg)
    code, msg = rc(8, 8, 8, 4, [1, 4])
    assert code == -1 and "class 4" in msg
    code, msg = rc(8, 8, 8, 80, list(range(65)))
    assert code == -1 and "reported classes" in msg
    for spacing in ((0.0, 1.0, 1.0), (1.0, 0.0, 1.0), (1.0, 1.0, 0.0), (1.0, -1.0, 1.0), (math.inf, 1.0, 1.0), (1.0, math.nan, 1.0)):
        code, msg = rc(8, 8, 8, 4, [1], spacing)
        assert code == -1 and "spacing" in msg, spacing
    code, msg = rc(8, 8, 8, 4, [1])  # every check passed: only the pointers are missing
    assert code == -1 and "null pointer" in msg


# ---- host side of the meter
def test_volume_meter_before_any_add_and_its_names():
    import spcl_amd  # noqa: F401
    from spcl_amd.contrastyou.meters import SurfaceMeter, VolumeSurfaceMeter
    for metername, abbr in (("hausdorff", "HD3D"), ("mod_hausdorff", "MHD3D"), ("average_surface", "ASD3D")):
        m = VolumeSurfaceMeter(C=4, report_axises=[1, 2, 3], metername=metername)
        means, stds = m.value()
        assert len(means) == 4 and len(stds) == 4 and all(math.isnan(v) for v in list(means) + list(stds))
        s = m.summary()
        assert list(s) == [f"{abbr}{i}" for i in (1, 2, 3)] and all(math.isnan(v) for v in s.values())
        assert m.get_plot_names() == list(s) and m.skipped_scans == 0 and "report_axis=[1, 2, 3]" in repr(m)
    with pytest.raises(AssertionError, match="`report_axises` should be either None or an iterator, given"):
        VolumeSurfaceMeter(C=4, report_axises=3)
    with pytest.raises(AssertionError):
        VolumeSurfaceMeter(C=4, metername="dice")
    assert SurfaceMeter.abbr == {"mod_hausdorff": "MHD", "hausdorff": "HD", "average_surface": "ASD"}  # untouched


def test_volume_meter_refuses_float_maps_cpu_tensors_and_batches_of_scans():
    import spcl_amd  # noqa: F401
    from spcl_amd import functional as F_hip
    from spcl_amd.contrastyou.meters import VolumeSurfaceMeter
    m = VolumeSurfaceMeter(C=2)
    with pytest.raises(TypeError, match="class-coded integer"):
        m.add(torch.zeros(3, 4, 4), torch.zeros(3, 4, 4))
    with pytest.raises(TypeError, match="class-coded integer"):
        m.add(torch.zeros(3, 2, 4, 4), torch.zeros(3, 2, 4, 4))  # a simplex is not taken
    with pytest.raises(TypeError, match="one scan"):
        m.add(torch.zeros(3, 2, 4, 4, dtype=torch.int64), torch.zeros(3, 2, 4, 4, dtype=torch.int64))
    with pytest.raises(AssertionError, match="incompatible shape"):
        m.add(torch.zeros(3, 4, 4, dtype=torch.int64), torch.zeros(3, 4, 5, dtype=torch.int64))
    vol = torch.zeros(3, 4, 4, dtype=torch.int64)
    with pytest.raises(RuntimeError, match="MI355X"):
        m.add(vol, vol)
    with pytest.raises(RuntimeError, match="MI355X"):
        F_hip.surface_distances_3d(vol, vol, 2)
    with pytest.raises(TypeError):
        F_hip.surface_distances_3d(vol.float(), vol.float(), 2)
    assert all(math.isnan(v) for v in m.value()[0]) and m._n == 0  # nothing was recorded


def test_inference_epocher_default_meter_set_is_unchanged():
    import inspect

    import spcl_amd  # noqa: F401
    from spcl_amd.contrastyou.losses.kl import KL_div
    from spcl_amd.contrastyou.meters import SurfaceMeter, VolumeSurfaceMeter
    from spcl_amd.semi_seg.epochers import InferenceEpocher
    from spcl_amd.semi_seg.trainers import FineTuneTrainer

    class _Net(torch.nn.Module):
        num_classes = 4

    def names(**kw):
        ep = InferenceEpocher(model=_Net(), loader=[], sup_criterion=KL_div(verbose=False), device="cpu", **kw)
        with ep.meters.focus_on("eval"):
            return ep, list(ep.meters._groups["eval"])

    ep, default = names()
    assert default == ["loss", "dice", "hd"] and names(volumetric=False)[1] == default
    with ep.meters.focus_on("eval"):
        assert type(ep.meters["hd"]) is SurfaceMeter and ep.meters["hd"]._report_axis == [1, 2, 3]
    ep, vol = names(volumetric=True, voxelspacing=(5.0, 1.25, 1.25))
    assert vol == ["loss", "dice", "hd", "hd3d", "mhd3d", "asd3d"]
    with ep.meters.focus_on("eval"):
        assert [type(ep.meters[k]) for k in vol[3:]] == [VolumeSurfaceMeter] * 3
        assert [ep.meters[k].get_plot_names()[0] for k in vol[3:]] == ["HD3D1", "MHD3D1", "ASD3D1"]
    sig = inspect.signature(FineTuneTrainer.inference).parameters
    assert sig["volumetric"].default is False and sig["voxelspacing"].default is None
    assert sig["volumetric"].kind is inspect.Parameter.KEYWORD_ONLY
