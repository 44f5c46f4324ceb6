"""``SurfaceMeter`` on the device against the meter oracle of tests/_surface_oracle.py (a batch with an empty reported class
is dropped, as the reference's raise + ``ExceptionIgnorer`` drops it).  Bars per recorded value as in
tests/test_gpu_surface_kernels.py (hd exact under unit spacing, mhd 16 eps d_max, asd (n + 8) eps d_max); a mean of such
values is held to the largest of their bars plus 2 eps d_max for the mean itself, the std to 1e-12 relative."""
import math

import numpy as np
import pytest
import torch

from tests import _surface_oracle as O

pytestmark = pytest.mark.gpu

C, REPORT, SHAPE = 4, [1, 2, 3], (4, 33, 40)
NAMES = ["hausdorff", "mod_hausdorff", "average_surface"]


@pytest.fixture(scope="module")
def batches():
    B, H, W = SHAPE
    return [(O.blob_maps(B, H, W, C, seed=70 + 2 * i), O.blob_maps(B, H, W, C, seed=71 + 2 * i)) for i in range(3)]


@pytest.fixture(scope="module")
def batches_with_a_hole(batches):
    out = [(p.copy(), t.copy()) for p, t in batches]
    out[1][0][2][out[1][0][2] == 3] = 0  # the middle batch: class 3 missing from one predicted slice
    return out


def _cuda(a):
    return torch.from_numpy(a).cuda()


def _bar(metername, batch_list):
    worst = 0.0
    for p, t in batch_list:
        o = O.surface_distances(p, t, C, REPORT)
        if o["empty"].any():
            continue
        dmax, n = o["hd"].max(), o["n"].max()
        worst = max(worst, {"hausdorff": 0.0, "mod_hausdorff": 16 * O.EPS * dmax,
                            "average_surface": (n + 8) * O.EPS * dmax}[metername] + 2 * O.EPS * dmax)
    return worst


def _compare(meter, metername, batch_list, skipped):
    mean, std, want_skipped, rows = O.meter(batch_list, C, REPORT, metername)
    assert want_skipped == skipped
    got_mean, got_std = meter.value()
    bar = _bar(metername, batch_list)
    print(f"{metername}: mean err {float(np.abs(got_mean - mean).max()):.3e} (bar {bar:.3e}), "
          f"std rel err {float((np.abs(got_std - std) / std).max()):.3e}")
    assert np.abs(np.asarray(got_mean) - mean).max() <= bar
    assert (np.abs(np.asarray(got_std) - std) <= 1e-12 * std).all()
    assert meter.skipped_batches == skipped
    abbr = {"hausdorff": "HD", "mod_hausdorff": "MHD", "average_surface": "ASD"}[metername]
    s = meter.summary()
    assert list(s) == [f"{abbr}{i}" for i in REPORT] and all(abs(s[f"{abbr}{c}"] - mean[k]) <= bar for k, c in enumerate(REPORT))


@pytest.mark.parametrize("metername", NAMES)
def test_meter_over_three_batches(batches, metername):
    import spcl_amd  # noqa: F401
    from spcl_amd.contrastyou.meters import SurfaceMeter
    m = SurfaceMeter(C=C, report_axises=REPORT, metername=metername)
    for p, t in batches:
        m.add(_cuda(p), _cuda(t))
    _compare(m, metername, batches, skipped=0)
    m.reset()
    assert all(math.isnan(v) for v in m.value()[0]) and m.skipped_batches == 0


@pytest.mark.parametrize("metername", NAMES)
def test_batch_with_an_empty_class_is_left_out(batches_with_a_hole, metername):
    import spcl_amd  # noqa: F401
    from spcl_amd.contrastyou.meters import SurfaceMeter
    m = SurfaceMeter(C=C, report_axises=REPORT, metername=metername)
    for p, t in batches_with_a_hole:
        m.add(_cuda(p), _cuda(t))
    _compare(m, metername, batches_with_a_hole, skipped=1)
    # the reference's ``add`` as it stands: raise, record nothing
    strict = SurfaceMeter(C=C, report_axises=REPORT, metername=metername)
    for i, (p, t) in enumerate(batches_with_a_hole):
        if i == 1:
            with pytest.raises(RuntimeError, match="does not contain any binary object"):
                strict.add(_cuda(p), _cuda(t), raise_on_empty=True)
        else:
            strict.add(_cuda(p), _cuda(t), raise_on_empty=True)
    assert strict._n == 2 and strict.skipped_batches == 0
    a, b = strict.value(), m.value()
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])


def test_simplex_and_one_hot_input_gives_the_class_coded_values(batches):
    import spcl_amd  # noqa: F401
    from spcl_amd.contrastyou.meters import SurfaceMeter
    p, t = (_cuda(a) for a in batches[0])
    onehot_t = torch.nn.functional.one_hot(t, C).permute(0, 3, 1, 2).contiguous()
    g = torch.Generator(device="cuda").manual_seed(3)
    prob = torch.rand((*p.shape, C), device="cuda", generator=g) * 0.2
    prob.scatter_(3, p.unsqueeze(3), 1.0)
    prob = (prob / prob.sum(3, keepdim=True)).permute(0, 3, 1, 2).contiguous()  # a simplex whose arg-max is p
    for name in NAMES:
        coded, hot = SurfaceMeter(C, REPORT, name), SurfaceMeter(C, REPORT, name)
        coded.add(p, t)
        hot.add(prob, onehot_t)
        assert np.array_equal(coded.value()[0], hot.value()[0]) and np.array_equal(coded.value()[1], hot.value()[1])
    spaced, plain = SurfaceMeter(C, REPORT), SurfaceMeter(C, REPORT)
    spaced.add(p, t, voxelspacing=2.0)
    plain.add(p, t)
    assert np.array_equal(spaced.value()[0], 2.0 * plain.value()[0])


def test_add_reads_nothing_back(batches):
    """``add`` runs under hipGraph capture on a side stream (as the validation graphs capture their batch): a device -> host
    copy or any other synchronising call inside it would fail the capture.  The first ``add`` of the shape runs eagerly --
    it allocates the cached workspace, which must not live in a graph's pool.  The replayed graph then yields the values."""
    import spcl_amd  # noqa: F401
    from spcl_amd.contrastyou.meters import SurfaceMeter
    p, t = (_cuda(a) for a in batches[0])
    m = SurfaceMeter(C=C, report_axises=REPORT, metername="average_surface")
    m.add(p, t)
    want = m.value()[0]
    m.reset()
    torch.cuda.synchronize()
    g, side = torch.cuda.CUDAGraph(), torch.cuda.Stream()
    with torch.cuda.graph(g, stream=side):
        m.add(p, t)
    g.replay()
    torch.cuda.synchronize()
    assert m._n == 1 and np.array_equal(m.value()[0], want)
