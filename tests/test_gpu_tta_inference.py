"""``InferenceEpocher(tta=...)`` and ``FineTuneTrainer.inference(tta=...)``: without the argument the pass is the one it was; with
it the plain meters and PNGs stay, the model sees the views of ``functional.tta_views`` in op order, and the merged maps
(PNGs under ``pred_tta/``, ``uncertainty_tta/``) are the float64 oracle of tests/_tta_oracle.py applied to the model's own
per-view logits.  Loader: the synthetic 'scans' of tests/test_gpu_lcc_inference.py (the image carries the label map).  The model
is NOT equivariant: it adds a fixed position-dependent ramp to label-derived logits, so the views disagree."""
import math
import os

import numpy as np
import pytest
import torch

from tests import _lcc_oracle as LCC
from tests import _tta_oracle as O

pytestmark = pytest.mark.gpu

C = 4
DISCS = ((1, 12, 12, 6), (2, 20, 28, 7), (3, 30, 14, 5))  # class, centre row, centre column, radius


def _scan(n, H, W, grow):
    yy, xx = np.mgrid[0:H, 0:W]
    vol = np.zeros((n, H, W), np.int64)
    for k in range(n):
        for c, cy, cx, r in DISCS:
            rr = r + (1 if grow and 0 < k < n - 1 else 0)
            vol[k][(yy - cy) ** 2 + (xx - cx) ** 2 <= rr * rr] = c
    return vol


class _Scans:
    def __init__(self, lengths, H, W):
        self.items = []
        for i, n in enumerate(lengths):
            tgt = torch.from_numpy(_scan(n, H, W, i % 2 == 0)).cuda().unsqueeze(1)
            names = [f"scan{i:02d}_{k:02d}" for k in range(n)]
            self.items.append(((tgt.float() / 4 + 0.1, tgt), names, ([0] * n, [f"scan{i:02d}"] * n)))

    def __len__(self):
        return len(self.items)

    def __iter__(self):
        return iter(self.items)


class _Ramp(torch.nn.Module):
    """logits = 2 at the label the image carries + a fixed ramp over the position IN THE FRAME THE MODEL IS CALLED IN, with no
    mirror or swap symmetry between its classes: the same pixel gets other logits in every view.  Records its inputs."""
    num_classes = C
    A = (2.9, -1.3, 0.7, -2.1)   # per class: slope along rows,
    B = (-1.7, 2.3, -0.9, 1.1)   # along columns,
    D = (0.37, -0.83, 1.9, -1.45)  # and of the product term

    def __init__(self, H, W):
        super().__init__()
        yy = (torch.arange(H, dtype=torch.float32) / H).view(H, 1).expand(H, W)
        xx = (torch.arange(W, dtype=torch.float32) / W).view(1, W).expand(H, W)
        ramp = torch.stack([a * yy + b * xx + d * yy * xx * xx for a, b, d in zip(self.A, self.B, self.D)])
        self.register_buffer("ramp", ramp.contiguous())
        self.seen = []

    def forward(self, img):
        self.seen.append(img.detach().clone())
        cls = (img.squeeze(1) * 4).long()
        onehot = torch.nn.functional.one_hot(cls, C).permute(0, 3, 1, 2).float()
        return (2 * onehot + self.ramp).contiguous()


def _png(path):
    from PIL import Image
    return np.asarray(Image.open(path)).astype(np.int64)


def _epocher(model, loader, save_dir, **kw):
    import spcl_amd  # noqa: F401
    from spcl_amd.contrastyou.losses.kl import KL_div
    from spcl_amd.semi_seg.epochers import InferenceEpocher
    ep = InferenceEpocher(model=model.cuda().eval(), loader=loader, sup_criterion=KL_div(verbose=False), device="cuda", **kw)
    ep.init(save_dir=str(save_dir))
    return ep


def _same(a, b):
    assert list(a) == list(b)
    assert np.array_equal(np.array(list(a.values()), float), np.array(list(b.values()), float), equal_nan=True), (a, b)


def _same_pngs(a, b, folders):
    for d in folders:
        assert sorted(os.listdir(a / d)) == sorted(os.listdir(b / d))
        for f in os.listdir(a / d):
            assert np.array_equal(_png(a / d / f), _png(b / d / f)), (d, f)


def _oracle_side(model, loader, mode):
    """per batch: the oracle's merge of the model's own logits for the oracle's views"""
    out = []
    with torch.no_grad():
        for (img, _), _, _ in loader:
            vs = O.views(img.cpu(), mode)
            logits = [model(v.cuda()).cpu() for v, _ in vs]
            out.append(O.merge(logits, [op for _, op in vs]))
    return out


def test_tta_none_is_the_pass_it_was(tmp_path):
    loader = _Scans([3, 4], 40, 48)
    plain = _epocher(_Ramp(40, 48), loader, tmp_path / "a").run()
    model = _Ramp(40, 48)
    none = _epocher(model, loader, tmp_path / "b", tta=None).run()
    assert list(plain) == list(none) == ["eval"] and list(plain["eval"]) == list(none["eval"]) == ["loss", "dice", "hd"]
    for k in plain["eval"]:
        _same(plain["eval"][k], none["eval"][k])
    for d in ("a", "b"):
        assert sorted(os.listdir(tmp_path / d)) == ["gt", "img", "pred"]
    _same_pngs(tmp_path / "a", tmp_path / "b", ("gt", "img", "pred"))
    assert len(model.seen) == len(loader)  # one forward per batch


def test_tta_flips(tmp_path):
    import spcl_amd  # noqa: F401
    from spcl_amd import functional as F_hip
    from spcl_amd.contrastyou.meters import SurfaceMeter, UniversalDice
    H, W = 40, 48
    loader = _Scans([3, 4, 2], H, W)
    plain_ep = _epocher(_Ramp(H, W), loader, tmp_path / "a")
    plain = plain_ep.run()
    model = _Ramp(H, W)
    ep = _epocher(model, loader, tmp_path / "b", tta="flips")
    stats = ep.run()
    assert list(stats["eval"]) == ["loss", "dice", "hd", "loss_tta", "dice_tta", "hd_tta", "tta_entropy", "tta_changed"]
    first = loader.items[0][0][0]
    views = F_hip.tta_views(first, "flips")
    assert [op for _, op in views] == [0, 1, 2, 3] and views[0][0] is first  # view 0 is the image itself, not a copy
    # the model saw the four flipped batches in op order, the plain batch first
    assert len(model.seen) == 4 * len(loader)
    for b, ((img, _), _, _) in enumerate(loader):
        assert torch.equal(model.seen[4 * b], img)
        for op in range(4):
            assert torch.equal(model.seen[4 * b + op].cpu(), O.view(img.cpu(), op)), (b, op)
    # the plain side is untouched
    for k in plain["eval"]:
        _same(plain["eval"][k], stats["eval"][k])
    assert ep.get_score() == plain_ep.get_score() == stats["eval"]["dice"]["DSC_mean"]
    assert sorted(os.listdir(tmp_path / "b")) == ["gt", "img", "pred", "pred_tta", "uncertainty_tta"]
    _same_pngs(tmp_path / "a", tmp_path / "b", ("gt", "img", "pred"))
    # the merged side against the oracle on the model's own per-view logits
    model.seen.clear()
    batches = _oracle_side(model, loader, "flips")
    gap = min(b[4] for b in batches)
    print(f"smallest top-two gap of the oracle's merge {gap:.3e}")
    assert gap >= 1e-4
    dice, hd = UniversalDice(C, report_axises=[1, 2, 3]), SurfaceMeter(C=C, report_axises=[1, 2, 3], metername="hausdorff")
    changed, entropies, losses = [], [], []
    for (prob, pred, entropy, mean_entropy, _), ((_, tgt), names, (_, group)) in zip(batches, loader):
        got = np.stack([_png(tmp_path / "b" / "pred_tta" / f"{n}.png") for n in names])
        assert np.array_equal(got, pred.numpy()), names
        unc = np.stack([_png(tmp_path / "b" / "uncertainty_tta" / f"{n}.png") for n in names])
        assert np.abs(unc - np.round(255 * entropy.numpy())).max() <= 1, names
        assert unc.max() > unc.min()
        plain_pred = np.stack([_png(tmp_path / "b" / "pred" / f"{n}.png") for n in names])
        changed.append(float((got != plain_pred).mean()))
        entropies.append(mean_entropy)
        t = tgt.squeeze(1).cpu()
        losses.append(float(-torch.log((prob.gather(1, t.unsqueeze(1)) + 1e-16) / (1 + 1e-16)).mean()))
        dice.add(pred.cuda(), t.cuda(), list(group))
        hd.add(pred.cuda(), t.cuda())
    _same(stats["eval"]["dice_tta"], dice.summary())
    _same(stats["eval"]["hd_tta"], hd.summary())
    got_changed, got_entropy = stats["eval"]["tta_changed"]["mean"], stats["eval"]["tta_entropy"]["mean"]
    got_loss = stats["eval"]["loss_tta"]["mean"]
    print(f"tta_changed {got_changed:.6f} / {np.mean(changed):.6f}, tta_entropy {got_entropy:.7f} / {np.mean(entropies):.7f}, "
          f"loss_tta {got_loss:.7f} / {np.mean(losses):.7f}")
    assert np.mean(changed) > 0 and abs(got_changed - np.mean(changed)) <= 1e-6  # the views really disagree
    # f32 probabilities (relative 1e-7) under a logarithm, averaged: the 1e-5 relative bar of the kernel tests
    assert math.isclose(got_entropy, np.mean(entropies), rel_tol=1e-5)
    assert math.isclose(got_loss, np.mean(losses), rel_tol=1e-5)


def test_tta_dihedral_volumetric_postprocess(tmp_path):
    H = W = 40
    loader = _Scans([3, 4], H, W)
    kw = dict(volumetric=True, postprocess="largest_component")
    plain_ep = _epocher(_Ramp(H, W), loader, tmp_path / "a", **kw)
    plain = plain_ep.run()
    model = _Ramp(H, W)
    ep = _epocher(model, loader, tmp_path / "b", tta="dihedral", **kw)
    stats = ep.run()
    old = ["loss", "dice", "hd", "hd3d", "mhd3d", "asd3d", "dice_lcc", "hd_lcc", "hd3d_lcc", "mhd3d_lcc", "asd3d_lcc", "lcc_removed"]
    new = ["loss_tta", "dice_tta", "hd_tta", "hd3d_tta", "mhd3d_tta", "asd3d_tta", "dice_tta_lcc", "hd_tta_lcc", "hd3d_tta_lcc",
           "mhd3d_tta_lcc", "asd3d_tta_lcc", "lcc_removed_tta", "tta_entropy", "tta_changed"]
    assert list(plain["eval"]) == old and list(stats["eval"]) == old + new
    assert [k for k in stats["eval"] if "tta" not in k] == old
    for k in old:
        _same(plain["eval"][k], stats["eval"][k])
    assert ep.get_score() == plain_ep.get_score() == stats["eval"]["dice"]["DSC_mean"]
    assert list(stats["eval"]["hd3d_tta"]) == list(stats["eval"]["hd3d_tta_lcc"]) == ["HD3D1", "HD3D2", "HD3D3"]
    assert sorted(os.listdir(tmp_path / "b")) == ["gt", "img", "pred", "pred_lcc", "pred_tta", "pred_tta_lcc", "uncertainty_tta"]
    _same_pngs(tmp_path / "a", tmp_path / "b", ("gt", "img", "pred", "pred_lcc"))
    assert len(model.seen) == 8 * len(loader)
    for b, ((img, _), _, _) in enumerate(loader):
        for op in range(8):
            assert torch.equal(model.seen[8 * b + op].cpu(), O.view(img.cpu(), op)), (b, op)
    model.seen.clear()
    batches = _oracle_side(model, loader, "dihedral")
    assert min(b[4] for b in batches) >= 1e-4
    removed = []
    for (_, pred, _, _, _), (_, names, _) in zip(batches, loader):
        got = np.stack([_png(tmp_path / "b" / "pred_tta" / f"{n}.png") for n in names])
        assert np.array_equal(got, pred.numpy()), names
        want = LCC.largest_components(got, C, volumetric=True)[0]
        lcc = np.stack([_png(tmp_path / "b" / "pred_tta_lcc" / f"{n}.png") for n in names])
        assert np.array_equal(lcc, want), names
        removed.append(LCC.removed_fraction(got, want))
    assert abs(stats["eval"]["lcc_removed_tta"]["mean"] - float(np.mean(removed))) <= 1e-6
    assert stats["eval"]["tta_changed"]["mean"] > 0


def test_trainer_inference_tta_from_best_checkpoint(tmp_path):
    import spcl_amd  # noqa: F401
    from spcl_amd.contrastyou.losses.kl import KL_div
    from spcl_amd.semi_seg.arch import UNet
    from spcl_amd.semi_seg.trainers import FineTuneTrainer
    from spcl_amd.synthetic import SyntheticLabeledLoader
    torch.manual_seed(0)
    model = UNet(input_dim=1, num_classes=4, max_channel=128)
    tra = SyntheticLabeledLoader(bs=4, size=32, device="cuda", seed=1)
    val = SyntheticLabeledLoader(bs=4, size=32, device="cuda", seed=1, twice=False, length=2)
    tr = FineTuneTrainer(model=model, labeled_loader=tra, val_loader=val, test_loader=val, criterion=KL_div(),
                         save_dir=str(tmp_path), max_epoch=1, num_batches=2, device="cuda", lr=2e-3, warmup_max=1,
                         multiplier=1)
    tr.init()
    tr.start_training()
    assert os.path.exists(tmp_path / "best.pth")
    plain, plain_score = tr.inference()
    assert list(plain["eval"]) == ["loss", "dice", "hd"] and not os.path.exists(tmp_path / "pred_tta")
    with pytest.raises(ValueError, match="tta"):
        tr.inference(tta="x")
    stats, score = tr.inference(tta="flips")
    assert list(stats["eval"]) == ["loss", "dice", "hd", "loss_tta", "dice_tta", "hd_tta", "tta_entropy", "tta_changed"]
    assert score == plain_score == stats["eval"]["dice"]["DSC_mean"]
    for k in plain["eval"]:
        _same(plain["eval"][k], stats["eval"][k])
    assert 0 < stats["eval"]["tta_entropy"]["mean"] <= 1 and 0 <= stats["eval"]["tta_changed"]["mean"] <= 1
    assert math.isfinite(stats["eval"]["loss_tta"]["mean"])
    n = len(os.listdir(tmp_path / "pred"))
    assert n == len(set(val.meta[0])) == len(os.listdir(tmp_path / "pred_tta")) == len(os.listdir(tmp_path / "uncertainty_tta"))
    dihedral = tr.inference(tta="dihedral")[0]  # (32 x 32 slices: square)
    assert list(dihedral["eval"]) == list(stats["eval"])
