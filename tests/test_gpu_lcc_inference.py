"""``InferenceEpocher(postprocess=...)`` and ``FineTuneTrainer.inference(postprocess=...)``: without the argument the pass is the
one it was; with ``"largest_component"`` the processed maps (PNGs under ``pred_lcc/``) are the scipy restatement of
tests/_lcc_oracle.py applied to the PNGs under ``pred/``, and the ``*_lcc`` meters are the project's meters over those maps.
Loader and model are the synthetic 'scans' of tests/test_gpu_surface3d_meter.py (the image carries the label map, the model's
arg-max reads it back shifted by one column) with stray islands planted into the prediction."""
import os

import numpy as np
import pytest
import torch

from tests import _lcc_oracle as O

pytestmark = pytest.mark.gpu

C, H, W = 4, 40, 48
DISCS = ((1, 12, 12, 6), (2, 20, 30, 7), (3, 30, 14, 5))  # class, centre row, centre column, radius


def _scan(n, grow):
    """[n, H, W]: one disc per foreground class in every slice (radius + 1 in the middle slices where ``grow``)"""
    yy, xx = np.mgrid[0:H, 0:W]
    vol = np.zeros((n, H, W), np.int64)
    for k in range(n):
        for c, cy, cx, r in DISCS:
            rr = r + (1 if grow and 0 < k < n - 1 else 0)
            vol[k][(yy - cy) ** 2 + (xx - cx) ** 2 <= rr * rr] = c
    return vol


class _Scans:
    def __init__(self, lengths):
        self.items = []
        for i, n in enumerate(lengths):
            tgt = torch.from_numpy(_scan(n, i % 2 == 0)).cuda().unsqueeze(1)
            names = [f"scan{i:02d}_{k:02d}" for k in range(n)]
            self.items.append(((tgt.float() / 4 + 0.1, tgt), names, ([0] * n, [f"scan{i:02d}"] * n)))

    def __len__(self):
        return len(self.items)

    def __iter__(self):
        return iter(self.items)


class _Lookup(torch.nn.Module):
    """arg-max = the label the image carries, shifted one column, plus islands far from their class: four voxels of class 1 in
    the far corner of the last slice, two of class 2 in the near corner of the first, and one voxel of class 3 that touches its
    disc only diagonally in the first slice"""
    num_classes = C

    def forward(self, img):
        cls = (img.squeeze(1) * 4).long().roll(1, dims=2)
        cls[-1, H - 3:H - 1, W - 4:W - 2] = 1
        cls[0, 1, 1:3] = 2
        cls[0, 30 - 5, 15 - 4] = 3  # (the shifted disc, radius 5 in a first slice, holds (-4, -3) but neither (-4, -4) nor (-5, -3))
        return torch.nn.functional.one_hot(cls, C).permute(0, 3, 1, 2).float().contiguous()


def _png(path):
    from PIL import Image
    return np.asarray(Image.open(path)).astype(np.int64)


def _epocher(loader, save_dir, **kw):
    import spcl_amd  # noqa: F401
    from spcl_amd.contrastyou.losses.kl import KL_div
    from spcl_amd.semi_seg.epochers import InferenceEpocher
    ep = InferenceEpocher(model=_Lookup().eval(), loader=loader, sup_criterion=KL_div(verbose=False), device="cuda", **kw)
    ep.init(save_dir=str(save_dir))
    return ep


def _same(a, b):
    assert list(a) == list(b)
    assert np.array_equal(np.array(list(a.values()), float), np.array(list(b.values()), float), equal_nan=True), (a, b)


def _oracle_side(loader, save_dir, volumetric):
    """per batch: (oracle-processed map, target, removed fraction) from the PNGs the pass wrote, checked against pred_lcc/"""
    out = []
    for (_, tgt), names, _ in loader:
        pred = np.stack([_png(save_dir / "pred" / f"{n}.png") for n in names])
        want = O.largest_components(pred, C, volumetric=volumetric)[0]
        got = np.stack([_png(save_dir / "pred_lcc" / f"{n}.png") for n in names])
        assert np.array_equal(got, want), names
        assert (want != pred).any()  # an island went in every batch
        out.append((want, tgt.squeeze(1).cpu().numpy(), O.removed_fraction(pred, want)))
    return out


def test_postprocess_none_is_the_pass_it_was(tmp_path):
    loader = _Scans([3, 4])
    plain = _epocher(loader, tmp_path / "a").run()
    none = _epocher(loader, tmp_path / "b", postprocess=None).run()
    assert list(plain) == list(none) == ["eval"] and list(plain["eval"]) == list(none["eval"]) == ["loss", "dice", "hd"]
    for k in plain["eval"]:
        _same(plain["eval"][k], none["eval"][k])
    for d in ("a", "b"):
        assert sorted(os.listdir(tmp_path / d)) == ["gt", "img", "pred"]
    for f in os.listdir(tmp_path / "a" / "pred"):
        assert np.array_equal(_png(tmp_path / "a" / "pred" / f), _png(tmp_path / "b" / "pred" / f))


def test_postprocess_largest_component_slice_wise(tmp_path):
    import spcl_amd  # noqa: F401
    from spcl_amd.contrastyou.meters import SurfaceMeter, UniversalDice
    loader = _Scans([3, 4, 2])
    plain_ep = _epocher(loader, tmp_path / "a")
    plain = plain_ep.run()
    ep = _epocher(loader, tmp_path / "b", postprocess="largest_component")
    stats = ep.run()
    assert list(stats["eval"]) == ["loss", "dice", "hd", "dice_lcc", "hd_lcc", "lcc_removed"]
    for k in plain["eval"]:  # the old keys keep their values
        _same(plain["eval"][k], stats["eval"][k])
    assert ep.get_score() == plain_ep.get_score() == stats["eval"]["dice"]["DSC_mean"]
    assert sorted(os.listdir(tmp_path / "b")) == ["gt", "img", "pred", "pred_lcc"]
    assert len(os.listdir(tmp_path / "b" / "pred_lcc")) == 9
    batches = _oracle_side(loader, tmp_path / "b", volumetric=False)
    dice, hd = UniversalDice(C, report_axises=[1, 2, 3]), SurfaceMeter(C=C, report_axises=[1, 2, 3], metername="hausdorff")
    for (want, tgt, _), (_, _, (_, group)) in zip(batches, loader):
        dice.add(torch.from_numpy(want).cuda(), torch.from_numpy(tgt).cuda(), list(group))
        hd.add(torch.from_numpy(want).cuda(), torch.from_numpy(tgt).cuda())
    _same(stats["eval"]["dice_lcc"], dice.summary())
    _same(stats["eval"]["hd_lcc"], hd.summary())
    assert stats["eval"]["dice_lcc"]["DSC_mean"] > stats["eval"]["dice"]["DSC_mean"]  # the islands were false positives
    want_removed = float(np.mean([f for _, _, f in batches]))
    got_removed = stats["eval"]["lcc_removed"]["mean"]
    print(f"lcc_removed {got_removed:.9f} against {want_removed:.9f}")
    assert 0 < want_removed < 0.05 and abs(got_removed - want_removed) <= 1e-6


def test_trainer_inference_volumetric_postprocess(tmp_path):
    import spcl_amd  # noqa: F401
    from spcl_amd.contrastyou.losses.kl import KL_div
    from spcl_amd.semi_seg.trainers import FineTuneTrainer
    model, loader = _Lookup(), _Scans([3, 5])
    tr = FineTuneTrainer(model=model, labeled_loader=loader, val_loader=loader, test_loader=loader, criterion=KL_div(verbose=False),
                         save_dir=str(tmp_path), max_epoch=1, num_batches=1, device="cuda")
    torch.save({"_model": model.state_dict()}, tmp_path / "best.pth")
    plain, plain_score = tr.inference(volumetric=True)
    assert list(plain["eval"]) == ["loss", "dice", "hd", "hd3d", "mhd3d", "asd3d"] and not os.path.exists(tmp_path / "pred_lcc")
    with pytest.raises(ValueError, match="postprocess"):
        tr.inference(volumetric=True, postprocess="x")
    stats, score = tr.inference(volumetric=True, postprocess="largest_component")
    assert list(stats["eval"]) == ["loss", "dice", "hd", "hd3d", "mhd3d", "asd3d", "dice_lcc", "hd_lcc", "hd3d_lcc", "mhd3d_lcc",
                                   "asd3d_lcc", "lcc_removed"]
    assert score == plain_score
    for k in plain["eval"]:
        _same(plain["eval"][k], stats["eval"][k])
    assert list(stats["eval"]["hd3d_lcc"]) == ["HD3D1", "HD3D2", "HD3D3"]
    assert list(stats["eval"]["mhd3d_lcc"]) == ["MHD3D1", "MHD3D2", "MHD3D3"]
    assert list(stats["eval"]["asd3d_lcc"]) == ["ASD3D1", "ASD3D2", "ASD3D3"]
    batches = _oracle_side(loader, tmp_path, volumetric=True)
    # per scan, the diagonal neighbour of the class-3 disc is a component of its own and went
    assert all(want[0, 25, 11] == 0 and want[0, 26, 12] == 3 for want, _, _ in batches)
    before, after = stats["eval"]["hd3d"], stats["eval"]["hd3d_lcc"]
    print(f"HD3D before {before}, after {after}")
    assert all(after[k] <= before[k] for k in before)
    assert after["HD3D1"] < before["HD3D1"] and before["HD3D1"] > 30 and after["HD3D1"] < 3  # the far corner island of class 1
    want_removed = float(np.mean([f for _, _, f in batches]))
    assert abs(stats["eval"]["lcc_removed"]["mean"] - want_removed) <= 1e-6
