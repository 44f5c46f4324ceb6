"""``VolumeSurfaceMeter`` on the device against the meter oracle of tests/_surface3d_oracle.py (a scan in which a reported
class is missing from the whole volume is dropped), the scan whose end slices are background only -- which the slice-wise
``SurfaceMeter`` drops and the volume meter reports --, and ``FineTuneTrainer.inference(volumetric=True)``.  Bars per recorded
value as in tests/test_gpu_surface3d_kernels.py (hd exact under unit spacing and 4 eps d_max with spacing, mhd 16 eps d_max,
asd (n + 8) eps d_max); a mean of such values is held to the largest of their bars plus 2 eps d_max for the mean itself, the
std to 1e-12 relative."""
import math
import os

import numpy as np
import pytest
import torch

from tests import _surface3d_oracle as O
from tests import _surface_oracle as O2

pytestmark = pytest.mark.gpu

C, REPORT, HW = 4, [1, 2, 3], (33, 40)
NAMES = ["hausdorff", "mod_hausdorff", "average_surface"]
ABBR = {"hausdorff": "HD3D", "mod_hausdorff": "MHD3D", "average_surface": "ASD3D"}
SPACING = (5.0, 1.25, 1.25)


@pytest.fixture(scope="module")
def scans():
    """four scans of different depth; class 3 is missing from the whole prediction of the third"""
    out = [(O.blob_volumes(1, D, *HW, C, seed=70 + 2 * i)[0], O.blob_volumes(1, D, *HW, C, seed=71 + 2 * i)[0])
           for i, D in enumerate((3, 5, 8, 4))]
    out[2][0][out[2][0] == 3] = 0
    return out


def _cuda(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _bar(metername, scan_list, spacing):
    worst = 0.0
    unit = O._spacing(spacing) == (1.0, 1.0, 1.0)
    for p, t in scan_list:
        o = O.surface_distances(p, t, C, REPORT, spacing)
        if o["empty"].any():
            continue
        dmax, n = o["hd"].max(), o["n"].max()
        worst = max(worst, {"hausdorff": 0.0 if unit else 4 * O.EPS * dmax, "mod_hausdorff": 16 * O.EPS * dmax,
                            "average_surface": (n + 8) * O.EPS * dmax}[metername] + 2 * O.EPS * dmax)
    return worst


@pytest.mark.parametrize("spacing", [None, SPACING])
@pytest.mark.parametrize("metername", NAMES)
def test_meter_over_scans_of_different_depth(scans, metername, spacing):
    import spcl_amd  # noqa: F401
    from spcl_amd.contrastyou.meters import VolumeSurfaceMeter
    m = VolumeSurfaceMeter(C=C, report_axises=REPORT, metername=metername)
    for i, (p, t) in enumerate(scans):
        if i % 2:
            m.add(_cuda(p).unsqueeze(1), _cuda(t).unsqueeze(1), voxelspacing=spacing)  # [D,1,H,W], as the loaders hand it over
        else:
            m.add(_cuda(p), _cuda(t), voxelspacing=spacing)
    mean, std, skipped, rows = O.meter(scans, C, REPORT, metername, spacing)
    assert skipped == 1 and rows.shape == (3, 3)
    got_mean, got_std = m.value()
    bar = _bar(metername, scans, spacing)
    print(f"{metername} spacing {spacing}: mean err {float(np.abs(got_mean - mean).max()):.3e} (bar {bar:.3e}), "
          f"std rel err {float((np.abs(got_std - std) / std).max()):.3e}")
    assert np.abs(np.asarray(got_mean) - mean).max() <= bar
    assert (np.abs(np.asarray(got_std) - std) <= 1e-12 * std).all()
    assert m.skipped_scans == 1 and m._n == 4
    s = m.summary()
    assert list(s) == [f"{ABBR[metername]}{i}" for i in REPORT] == m.get_plot_names()
    assert all(abs(s[f"{ABBR[metername]}{c}"] - mean[k]) <= bar for k, c in enumerate(REPORT))
    # the reference's ``add`` as it stands: raise, record nothing
    strict = VolumeSurfaceMeter(C=C, report_axises=REPORT, metername=metername)
    for i, (p, t) in enumerate(scans):
        if i == 2:
            with pytest.raises(RuntimeError, match="does not contain any binary object"):
                strict.add(_cuda(p), _cuda(t), voxelspacing=spacing, raise_on_empty=True)
        else:
            strict.add(_cuda(p), _cuda(t), voxelspacing=spacing, raise_on_empty=True)
    assert strict._n == 3 and strict.skipped_scans == 0
    assert np.array_equal(strict.value()[0], got_mean) and np.array_equal(strict.value()[1], got_std)
    m.reset()
    assert all(math.isnan(v) for v in m.value()[0]) and m.skipped_scans == 0


def test_scan_with_background_end_slices(scans):
    """first and last slice background only: slice-wise a reported class is missing from a slice, so the whole batch is left
    out; the volume holds every class and is reported"""
    import spcl_amd  # noqa: F401
    from spcl_amd.contrastyou.meters import SurfaceMeter, VolumeSurfaceMeter
    pred, target = (np.concatenate([np.zeros((1, *HW), np.int64), a, np.zeros((1, *HW), np.int64)]) for a in scans[1])
    assert all((a[1:-1] == c).any() for a in (pred, target) for c in REPORT)
    for metername in NAMES:
        flat, vol = SurfaceMeter(C, REPORT, metername), VolumeSurfaceMeter(C, REPORT, metername)
        flat.add(_cuda(pred), _cuda(target))
        vol.add(_cuda(pred), _cuda(target), voxelspacing=SPACING)
        assert flat.skipped_batches == 1 and all(math.isnan(v) for v in flat.summary().values())
        assert O2.meter([(pred, target)], C, REPORT, metername)[2] == 1  # (the slice-wise oracle drops it too)
        mean, _, skipped, rows = O.meter([(pred, target)], C, REPORT, metername, SPACING)
        assert skipped == 0 and rows.shape == (1, 3) and np.isfinite(mean).all() and (mean > 0).all()
        got = np.array(list(vol.summary().values()))
        bar = _bar(metername, [(pred, target)], SPACING)
        print(f"{metername}: {got} against {mean}, err {float(np.abs(got - mean).max()):.3e} (bar {bar:.3e})")
        assert vol.skipped_scans == 0 and np.isfinite(got).all() and np.abs(got - mean).max() <= bar


def test_add_reads_nothing_back(scans):
    """``add`` under hipGraph capture on a side stream: a device -> host copy or any other synchronising call inside it would
    fail the capture.  The first ``add`` of the shape runs eagerly (it allocates the cached workspace)."""
    import spcl_amd  # noqa: F401
    from spcl_amd.contrastyou.meters import VolumeSurfaceMeter
    p, t = (_cuda(a) for a in scans[0])
    m = VolumeSurfaceMeter(C=C, report_axises=REPORT, metername="average_surface")
    m.add(p, t, voxelspacing=SPACING)
    want = m.value()[0]
    m.reset()
    torch.cuda.synchronize()
    g, side = torch.cuda.CUDAGraph(), torch.cuda.Stream()
    with torch.cuda.graph(g, stream=side):
        m.add(p, t, voxelspacing=SPACING)
    g.replay()
    torch.cuda.synchronize()
    assert m._n == 1 and np.array_equal(m.value()[0], want)


# ---- the trainer
class _Scans:
    """finite, re-iterable loader of the kind of tests/test_gpu_inference_epocher.py: one 'scan' (a batch of its own slice
    count) per item, single-transform format; the image carries the label map (class / 4 + 0.1)"""

    def __init__(self, lengths, size=40):
        self.items = []
        for i, n in enumerate(lengths):
            tgt = torch.from_numpy(O.blob_volumes(1, n, size, size + 8, C, seed=90 + i)[0]).cuda().unsqueeze(1)
            names = [f"scan{i:02d}_{k:02d}" for k in range(n)]
            self.items.append(((tgt.float() / 4 + 0.1, tgt), names, ([0] * n, [f"scan{i:02d}"] * n)))

    def __len__(self):
        return len(self.items)

    def __iter__(self):
        return iter(self.items)


class _Lookup(torch.nn.Module):
    """arg-max = the label the image carries, shifted one column and, from the second slice on, one row: a prediction that
    holds every class of the scan at a non-zero distance"""
    num_classes = C

    def forward(self, img):
        cls = (img.squeeze(1) * 4).long().roll(1, dims=2)
        cls[1:] = cls[1:].roll(1, dims=1)
        return torch.nn.functional.one_hot(cls, C).permute(0, 3, 1, 2).float().contiguous()


def _png(path):
    from PIL import Image
    return np.asarray(Image.open(path))


def test_trainer_inference_volumetric(tmp_path):
    import spcl_amd  # noqa: F401
    from spcl_amd.contrastyou.losses.kl import KL_div
    from spcl_amd.semi_seg.trainers import FineTuneTrainer
    from spcl_amd.synthetic import SyntheticLabeledLoader
    model, loader = _Lookup(), _Scans([3, 6, 4])
    tr = FineTuneTrainer(model=model, labeled_loader=loader, val_loader=loader, test_loader=loader, criterion=KL_div(verbose=False),
                         save_dir=str(tmp_path), max_epoch=1, num_batches=1, device="cuda")
    torch.save({"_model": model.state_dict()}, tmp_path / "best.pth")
    plain, plain_score = tr.inference()
    assert list(plain) == ["eval"] and list(plain["eval"]) == ["loss", "dice", "hd"]  # the parent commit's keys
    assert list(plain["eval"]["hd"]) == ["HD1", "HD2", "HD3"]
    stats, score = tr.inference(volumetric=True, voxelspacing=SPACING)
    assert list(stats["eval"]) == ["loss", "dice", "hd", "hd3d", "mhd3d", "asd3d"] and score == plain_score
    for k in ("loss", "dice", "hd"):  # what was there is what it was, bit for bit (NaN where a slice lacks a class)
        assert list(stats["eval"][k]) == list(plain["eval"][k])
        assert np.array_equal(np.array(list(stats["eval"][k].values())), np.array(list(plain["eval"][k].values())),
                              equal_nan=True)
    # the oracle on the PNGs the pass wrote, stacked per scan in file-name order
    volumes = []
    for i, ((_, _), names, _) in enumerate(loader):
        assert names == sorted(names)
        volumes.append((np.stack([_png(tmp_path / "pred" / f"{n}.png") for n in names]).astype(np.int64),
                        np.stack([_png(tmp_path / "gt" / f"{n}.png") for n in names]).astype(np.int64)))
    for key, metername in (("hd3d", "hausdorff"), ("mhd3d", "mod_hausdorff"), ("asd3d", "average_surface")):
        mean, _, skipped, rows = O.meter(volumes, C, REPORT, metername, SPACING)
        assert skipped == 0 and rows.shape == (3, 3) and (mean > 0).all()
        got = stats["eval"][key]
        assert list(got) == [f"{ABBR[metername]}{c}" for c in REPORT]
        bar = _bar(metername, volumes, SPACING)
        err = max(abs(got[f"{ABBR[metername]}{c}"] - mean[k]) for k, c in enumerate(REPORT))
        print(f"{key}: {got}, err {err:.3e} (bar {bar:.3e})")
        assert err <= bar
    # a loader batch that mixes two scan names is not a volume
    mixed = SyntheticLabeledLoader(bs=4, size=32, device="cuda", seed=1, twice=False, length=1)
    assert len(set(mixed.meta[2])) == 2
    tr2 = FineTuneTrainer(model=model, labeled_loader=mixed, val_loader=mixed, test_loader=mixed, criterion=KL_div(verbose=False),
                          save_dir=str(tmp_path), max_epoch=1, num_batches=1, device="cuda")
    with pytest.raises(ValueError, match="mixes"):
        tr2.inference(volumetric=True, voxelspacing=SPACING)
    assert set(tr2.inference()[0]["eval"]) == {"loss", "dice", "hd"}  # (without the flag such a loader is served as before)
    assert os.path.exists(tmp_path / "pred" / f"{mixed.meta[0][0]}.png")
