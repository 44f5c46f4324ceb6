"""``InferenceEpocher`` (loss + Dice as ``EvalEpocher``, the Hausdorff meter, PNGs of image / label / prediction) and
``FineTuneTrainer.inference`` (semi_seg/epochers/base.py:93-125, semi_seg/trainers/base.py:127-148).  Model and loader are
the small ones of tests/test_gpu_eval_graph.py: a 128-channel UNet on 'scans' of 64 x 64 slices."""
import os

import numpy as np
import pytest
import torch

from tests import _surface_oracle as O

pytestmark = pytest.mark.gpu


class _Scans:
    """finite, re-iterable loader: one 'scan' (a batch of its own slice count) per item, single-transform format"""

    def __init__(self, lengths, size=64, seed=5, classes=4):
        g = torch.Generator(device="cuda").manual_seed(seed)
        self.items = []
        for i, n in enumerate(lengths):
            img = torch.rand((n, 1, size, size), device="cuda", generator=g)
            coarse = torch.randint(0, classes, (n, 1, size // 8, size // 8), device="cuda", generator=g)
            tgt = torch.nn.functional.interpolate(coarse.float(), size=(size, size), mode="nearest").long()
            names = [f"scan{i:02d}_{k:02d}" for k in range(n)]
            self.items.append(((img, tgt), names, ([0] * n, [f"scan{i:02d}"] * n)))

    def __len__(self):
        return len(self.items)

    def __iter__(self):
        return iter(self.items)


def _model():
    import spcl_amd  # noqa: F401
    from spcl_amd.semi_seg.arch import UNet
    torch.manual_seed(21)
    m = UNet(input_dim=1, num_classes=4, max_channel=128).cuda()
    m.set_compute_dtype(torch.float32)
    return m


def _png(path):
    from PIL import Image
    return np.asarray(Image.open(path))


def test_inference_epocher_meters_and_pngs(tmp_path):
    from spcl_amd import functional as F_hip
    from spcl_amd.contrastyou.losses.kl import KL_div
    from spcl_amd.semi_seg.epochers import EvalEpocher, InferenceEpocher
    model, loader = _model(), _Scans([3, 5, 3, 4])
    ref = EvalEpocher(model=model, loader=loader, sup_criterion=KL_div(verbose=False), device="cuda", graph=False)
    ref_stats = ref.run()
    ep = InferenceEpocher(model=model, loader=loader, sup_criterion=KL_div(verbose=False), device="cuda")
    with pytest.raises(RuntimeError, match="save_dir"):
        ep.run()
    ep = InferenceEpocher(model=model, loader=loader, sup_criterion=KL_div(verbose=False), device="cuda")
    ep.init(save_dir=str(tmp_path))
    stats = ep.run()
    assert list(stats) == ["eval"] and list(stats["eval"]) == ["loss", "dice", "hd"]
    # loss and Dice: EvalEpocher's, bit for bit
    assert stats["eval"]["loss"] == ref_stats["eval"]["loss"] and stats["eval"]["dice"] == ref_stats["eval"]["dice"]
    assert ep.get_score() == ref.get_score() == stats["eval"]["dice"]["DSC_mean"]
    with ep.meters.focus_on("eval"), ref.meters.focus_on("eval"):
        assert torch.equal(torch.cat(ep.meters["dice"]._intersections), torch.cat(ref.meters["dice"]._intersections))
        assert torch.equal(torch.cat(ep.meters["dice"]._unions), torch.cat(ref.meters["dice"]._unions))
        hd_meter = ep.meters["hd"]
    # hd: the meter oracle on the arg-max maps read back
    model.eval()
    batches = []
    with torch.no_grad():
        for (img, tgt), names, _ in loader:
            pred = F_hip.argmax_classes(model(img))
            batches.append((pred.cpu().numpy(), tgt.squeeze(1).cpu().numpy(), img, names))
    mean, _, skipped, rows = O.meter([(p, t) for p, t, _, _ in batches], 4, [1, 2, 3], "hausdorff")
    print(f"hd rows recorded {rows.shape[0]}, batches skipped {skipped} of {len(batches)}: {stats['eval']['hd']}")
    assert hd_meter.skipped_batches == skipped and list(stats["eval"]["hd"]) == ["HD1", "HD2", "HD3"]
    got = np.array([stats["eval"]["hd"][f"HD{c}"] for c in (1, 2, 3)])
    assert np.array_equal(np.isnan(got), np.isnan(mean))
    if not np.isnan(mean).any():  # (unit spacing: every recorded value is exact, and so is their mean)
        assert np.array_equal(got, mean), (got, mean)
    # PNGs: one per slice and folder, decoded contents = the tensors
    total = sum(len(n) for _, _, _, n in batches)
    for folder in ("img", "gt", "pred"):
        assert len(os.listdir(tmp_path / folder)) == total
    for pred, tgt, img, names in batches:
        img255 = (img.squeeze(1) * 255).to(torch.uint8).cpu().numpy()
        for k, name in enumerate(names):
            assert np.array_equal(_png(tmp_path / "img" / f"{name}.png"), img255[k])
            assert np.array_equal(_png(tmp_path / "gt" / f"{name}.png"), tgt[k].astype(np.uint8))
            assert np.array_equal(_png(tmp_path / "pred" / f"{name}.png"), pred[k].astype(np.uint8))
            assert _png(tmp_path / "pred" / f"{name}.png").dtype == np.uint8


def test_inference_epocher_records_hausdorff_when_every_class_is_predicted(tmp_path):
    """a model whose arg-max reproduces a given label map (the image carries the label; the class map is a fixed function of
    it) predicts every foreground class in every slice: no batch is left out, and ``hd`` is the oracle's mean"""
    from spcl_amd.contrastyou.losses.kl import KL_div
    from spcl_amd.semi_seg.epochers import InferenceEpocher

    class _Lookup(torch.nn.Module):
        num_classes = 4

        def forward(self, img):  # img = class / 4 + 0.1: logits peak at the class, shifted one column for a non-zero distance
            cls = (img.squeeze(1) * 4).long().roll(1, dims=2)
            return torch.nn.functional.one_hot(cls, 4).permute(0, 3, 1, 2).float().contiguous()

    items = []
    for i, n in enumerate((2, 3)):
        tgt = torch.from_numpy(O.blob_maps(n, 40, 48, 4, seed=90 + i)).cuda().unsqueeze(1)
        items.append(((tgt.float() / 4 + 0.1, tgt), [f"s{i}_{k}" for k in range(n)], ([0] * n, [f"s{i}"] * n)))
    ep = InferenceEpocher(model=_Lookup(), loader=items, sup_criterion=KL_div(verbose=False), device="cuda")
    ep.init(save_dir=str(tmp_path))
    stats = ep.run()
    pairs = [(t.squeeze(1).roll(1, dims=2).cpu().numpy(), t.squeeze(1).cpu().numpy()) for (_, t), _, _ in items]
    mean, _, skipped, rows = O.meter(pairs, 4, [1, 2, 3], "hausdorff")
    assert skipped == 0 and rows.shape == (5, 3) and (mean > 0).all()
    assert np.array_equal(np.array([stats["eval"]["hd"][f"HD{c}"] for c in (1, 2, 3)]), mean)
    with ep.meters.focus_on("eval"):
        assert ep.meters["hd"].skipped_batches == 0


def test_trainer_inference_loads_best_checkpoint(tmp_path):
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
                         save_dir=str(tmp_path), max_epoch=1, num_batches=4, device="cuda", lr=2e-3, warmup_max=1,
                         multiplier=1)
    tr.init()
    tr.start_training()
    assert os.path.exists(tmp_path / "best.pth")
    best = torch.load(tmp_path / "best.pth", map_location="cpu")["_model"]
    with torch.no_grad():
        for p in model.parameters():
            p.add_(0.5)  # (inference must put the checkpoint's weights back)
    stats, score = tr.inference()
    assert score == stats["eval"]["dice"]["DSC_mean"] and set(stats["eval"]) == {"loss", "dice", "hd"}
    for k, v in model.state_dict().items():
        assert torch.equal(v.cpu(), best[k]), k
    assert abs(score - tr.history[-1]["score"]) < 1e-6  # the validation score of the epoch that wrote best.pth
    assert len(os.listdir(tmp_path / "pred")) == len(set(val.meta[0]))
    # a .pth file, a directory holding best.pth, and what is neither
    assert tr.inference(str(tmp_path / "best.pth"))[1] == score and tr.inference(str(tmp_path))[1] == score
    wrong = tmp_path / "best.ckpt"
    wrong.write_bytes(b"x")
    with pytest.raises(FileNotFoundError):
        tr.inference(str(wrong))
    with pytest.raises(FileNotFoundError):
        tr.inference(str(tmp_path / "nowhere"))
