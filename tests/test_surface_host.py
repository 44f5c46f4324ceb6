"""CPU-only: the surface-distance oracle (tests/_surface_oracle.py) against an all-pairs brute force and against answers
worked out by hand; the host side of ``SurfaceMeter`` (constructor assertions, the NaN pair before any ``add``, plot names)
and the refusal of CPU tensors."""
import math

import numpy as np
import pytest
import torch

from tests import _surface_oracle as O

SHAPES = [(1, 1), (1, 7), (5, 1), (7, 9), (17, 33), (64, 64), (65, 70)]


@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("spacing", [None, (1.25, 0.7)])
def test_oracle_equals_brute_force(shape, spacing):
    rng = np.random.RandomState(shape[0] * 131 + shape[1])
    for density in (0.05, 0.3, 0.6, 0.95):
        a, b = rng.rand(*shape) < density, rng.rand(*shape) < density
        a.flat[rng.randint(a.size)] = True  # (an empty mask raises: tested below)
        b.flat[rng.randint(b.size)] = True
        for x, y in ((a, b), (b, a)):
            got, want = np.sort(O.directed(x, y, spacing)), np.sort(O.directed_brute(x, y, spacing))
            assert got.shape == want.shape and np.array_equal(got, want), float(np.abs(got - want).max())
        assert O.hausdorff(a, b, spacing) == O.hausdorff(a, b, spacing, directed_fn=O.directed_brute)
        assert O.mod_hausdorff(a, b, spacing) == O.mod_hausdorff(a, b, spacing, directed_fn=O.directed_brute)
        assert abs(O.average_surface(a, b, spacing) - O.average_surface(a, b, spacing, directed_fn=O.directed_brute)) \
            <= 4 * O.EPS * O.hausdorff(a, b, spacing)  # (the sums run over differently ordered lists)


@pytest.mark.parametrize("k", [1, 4, 9])
@pytest.mark.parametrize("spacing", [None, 2.0, (1.25, 0.7)])
def test_single_pixel_against_single_pixel(k, spacing):
    a, b = np.zeros((3, 12), bool), np.zeros((3, 12), bool)
    a[1, 1], b[1, 1 + k] = True, True
    sx = O._spacing(spacing)[1]
    for fn in (O.hausdorff, O.mod_hausdorff, O.average_surface):
        assert fn(a, b, spacing) == k * sx


def test_identical_masks_give_zero():
    m = O.blob_maps(1, 17, 33, 3, seed=3)[0] == 1
    assert O.hausdorff(m, m) == 0.0 and O.mod_hausdorff(m, m) == 0.0 and O.average_surface(m, m) == 0.0


def test_border_of_a_full_image_is_the_frame_and_a_pixel_is_its_own_border():
    full = np.ones((6, 8), bool)
    frame = full.copy()
    frame[1:-1, 1:-1] = False
    assert np.array_equal(O.border(full), frame)
    one = np.zeros((5, 5), bool)
    one[2, 3] = True
    assert np.array_equal(O.border(one), one)
    assert np.array_equal(O.border(np.ones((1, 1), bool)), np.ones((1, 1), bool))


def test_square_inside_square():
    """3 x 3 inside 5 x 5, concentric: the 8 border pixels of the small one are all at distance 1 from the large ring; of the
    16 ring pixels of the large one the 4 corners are sqrt(2) from the small ring, the other 12 at distance 1"""
    a, b = np.zeros((9, 9), bool), np.zeros((9, 9), bool)
    a[3:6, 3:6], b[2:7, 2:7] = True, True
    assert int(O.border(a).sum()) == 8 and int(O.border(b).sum()) == 16
    assert np.array_equal(np.sort(O.directed(a, b)), np.ones(8))
    assert np.array_equal(np.sort(O.directed(b, a)), np.array([1.0] * 12 + [math.sqrt(2.0)] * 4))
    assert O.hausdorff(a, b) == math.sqrt(2.0)
    assert O.mod_hausdorff(a, b) == math.sqrt(2.0)  # n = 16: virtual index 14.25, both neighbours are sqrt(2)
    assert abs(O.average_surface(a, b) - (1.0 + (12.0 + 4.0 * math.sqrt(2.0)) / 16.0) / 2.0) < 4 * O.EPS


def test_percentile_with_integral_and_fractional_virtual_index():
    a, b = O.line_against_pixel(21)  # distances 3 .. 23; (21 - 1) * 0.95 = 19 -> the 20th value
    assert np.array_equal(np.sort(O.directed(a, b)), np.arange(3.0, 24.0))
    assert O.mod_hausdorff(a, b, percentile=95) == 22.0
    a, b = O.line_against_pixel(20)  # distances 3 .. 22; (20 - 1) * 0.95 = 18.05 -> 21 + 0.05 * (22 - 21)
    assert abs(O.mod_hausdorff(a, b, percentile=95) - 21.05) < 16 * O.EPS * 22.0
    assert O.mod_hausdorff(a, b, percentile=50) == 12.5
    assert O.hausdorff(a, b) == 22.0 and O.average_surface(a, b) == (12.5 + 3.0) / 2.0


def test_empty_mask_raises_and_the_meter_oracle_drops_the_batch():
    a, e = np.ones((3, 3), bool), np.zeros((3, 3), bool)
    for x, y in ((a, e), (e, a), (e, e)):
        with pytest.raises(RuntimeError):
            O.directed(x, y)
    full = O.blob_maps(2, 9, 11, 3, seed=1)
    holed = full.copy()
    holed[1][holed[1] == 2] = 0
    mean, std, skipped, rows = O.meter([(full, full), (holed, full), (full, O.blob_maps(2, 9, 11, 3, seed=2))], 3, [1, 2],
                                       "hausdorff")
    assert skipped == 1 and rows.shape == (4, 2) and np.array_equal(rows[:2], np.zeros((2, 2)))
    assert np.array_equal(mean, rows.mean(0)) and np.array_equal(std, rows.std(0))


# ---- host side of the meter
def test_surface_meter_constructor_assertions():
    import spcl_amd  # noqa: F401
    from spcl_amd.contrastyou.meters import SurfaceMeter
    with pytest.raises(AssertionError, match="`report_axises` should be either None or an iterator, given"):
        SurfaceMeter(C=4, report_axises=3)
    with pytest.raises(AssertionError, match="Incompatible parameter of `C`=4 and `report_axises`="):
        SurfaceMeter(C=4, report_axises=[1, 5])
    with pytest.raises(AssertionError):
        SurfaceMeter(C=4, metername="dice")
    assert set(SurfaceMeter.meter_choices) == {"mod_hausdorff", "hausdorff", "average_surface"}
    assert SurfaceMeter.abbr == {"mod_hausdorff": "MHD", "hausdorff": "HD", "average_surface": "ASD"}


def test_surface_meter_before_any_add():
    import spcl_amd  # noqa: F401
    from spcl_amd.contrastyou.meters import SurfaceMeter
    m = SurfaceMeter(C=4, report_axises=[1, 2, 3])
    means, stds = m.value()
    assert len(means) == 4 and len(stds) == 4 and all(math.isnan(v) for v in list(means) + list(stds))
    s = m.summary()
    assert list(s) == ["HD1", "HD2", "HD3"] and all(math.isnan(v) for v in s.values())
    assert m.skipped_batches == 0
    assert "report_axis=[1, 2, 3]" in repr(m)


@pytest.mark.parametrize("metername,abbr", [("hausdorff", "HD"), ("mod_hausdorff", "MHD"), ("average_surface", "ASD")])
def test_surface_meter_plot_names(metername, abbr):
    import spcl_amd  # noqa: F401
    from spcl_amd.contrastyou.meters import SurfaceMeter
    assert SurfaceMeter(C=4, report_axises=[1, 3], metername=metername).get_plot_names() == [f"{abbr}1", f"{abbr}3"]
    assert SurfaceMeter(C=3, metername=metername).get_plot_names() == [f"{abbr}{i}" for i in range(3)]


def test_cpu_tensors_are_refused():
    import spcl_amd  # noqa: F401
    from spcl_amd import functional as F_hip
    from spcl_amd.contrastyou.meters import SurfaceMeter
    pred = torch.zeros(1, 4, 4, dtype=torch.int64)
    with pytest.raises(RuntimeError, match="MI355X"):
        F_hip.surface_distances(pred, pred, 2)
    m = SurfaceMeter(C=2)
    with pytest.raises(RuntimeError, match="MI355X"):
        m.add(pred, pred)
    with pytest.raises(AssertionError, match="incompatible shape"):
        m.add(pred, torch.zeros(1, 4, 5, dtype=torch.int64))
    assert all(math.isnan(v) for v in m.value()[0])  # nothing was recorded


def test_inference_names_resolve():
    import spcl_amd  # noqa: F401
    from spcl_amd.semi_seg import epochers
    from spcl_amd.semi_seg.epochers import helper
    from spcl_amd.semi_seg.trainers import FineTuneTrainer, SemiTrainer
    assert issubclass(epochers.InferenceEpocher, epochers.EvalEpocher)
    assert callable(helper.write_predict) and callable(helper.write_img_target)
    assert callable(FineTuneTrainer.inference) and SemiTrainer.inference is FineTuneTrainer.inference
