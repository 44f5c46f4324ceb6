"""GPU: the label-guided pixel-contrast hook (semi_seg/hooks/pixelcontrast.py) on the tiny UNet of
tests/test_gpu_semi_reg_hooks.py: 2 + 2 slices of 64 x 64, 4 classes, 16 samples per class, ``Up_conv3`` (32 x 32 cells).

One ``SemiSupervisedEpocher.step`` returns ``weight *`` the loss the functional pipeline gives when it is run again on the
recorded feature, label maps and seed word (the same bits), and the meters hold what ``count`` says.  The gradient reaches the
head and the UNet up to the hooked feature and nothing behind it.  ``draw`` advances by one per step with synchronising calls
forbidden.  With ``unlabeled_threshold`` cells of unlabelled slices are sampled.  Two seeded ``SemiTrainer`` runs end with
identical parameters and ``draw``; a ``state_dict()`` round trip restores ``draw`` and the next step.  Without the section a
trainer is what it was.  A label batch of one class gives loss 0 and a finite step."""
import io
import random

import numpy as np
import pytest
import torch

from tests import _pixel_contrast_oracle as O
from tests.test_gpu_pseudo_label_hooks import _cfg, _trainer
from tests.test_gpu_semi_reg_hooks import MT, _drive, _setup, _snapshot, _unet
from tests.test_gpu_semi_step import _batch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
PC = {"weight": 0.5, "samples_per_class": 16, "seed": 11}


def _blocky(batch, seed, classes=4):
    """the batch with label maps of 8 x 8 blocks: every 2 x 2 pooling window of ``Up_conv3`` is pure"""
    (img, img_tf, tgt, _), names, groups = batch
    g = torch.Generator().manual_seed(seed)
    n, _, size, _ = tgt.shape
    coarse = torch.randint(0, classes, (n, 1, size // 8, size // 8), generator=g)
    t = coarse.repeat_interleave(8, 2).repeat_interleave(8, 3)
    return (img, img_tf, t, t.clone()), names, groups


def _spy(monkeypatch):
    """record what the hook hands to the sampler and to its criterion pipeline, and what they return"""
    from spcl_amd import functional as F_hip
    from spcl_amd.semi_seg.hooks import pixelcontrast
    seen = {}
    real_sample = F_hip.pixel_sample
    real_crit = pixelcontrast._PixelContrastEpocherHook.criterion_of

    def sample(cell_label, C, K, seed):
        seen.update(cell_label=cell_label.clone(), C=C, K=K, word=seed.clone())
        idx, count = real_sample(cell_label, C, K, seed)
        seen.update(idx=idx.clone(), count=count.clone())
        return idx, count

    def criterion_of(self, feature, idx, count):
        loss = real_crit(self, feature, idx, count)
        seen.update(feature=feature.detach().clone(), loss=loss.detach().clone())
        return loss

    monkeypatch.setattr(F_hip, "pixel_sample", sample)
    monkeypatch.setattr(pixelcontrast._PixelContrastEpocherHook, "criterion_of", criterion_of)
    return seen, real_sample, real_crit


def test_step_returns_the_functional_pipeline_of_its_own_feature(monkeypatch):
    from spcl_amd import functional as F_hip
    from spcl_amd.semi_seg.hooks import PixelContrastTrainerHook
    sd, model, hook, ep, flat = _setup("PixelContrastParameters", PC, lr=0.0)  # (lr 0: the head is the same afterwards)
    assert isinstance(hook, PixelContrastTrainerHook) and hook.draw.is_cuda and hook.draw.tolist() == [11]
    seen, real_sample, real_crit = _spy(monkeypatch)
    lab, unl = _blocky(_batch(2, 64, 1), 5), _batch(2, 64, 2)
    with ep.meters.focus_on(ep.meter_focus):
        sup, reg = ep.step(lab, unl, seed=1234)
    torch.cuda.synchronize()
    assert seen["C"] == 4 and seen["K"] == 16 and seen["word"].tolist() == [11] and hook.draw.tolist() == [12]
    assert tuple(seen["feature"].shape) == (2, model.get_channel_dim("Up_conv3"), 32, 32)  # the labelled rows only
    target = lab[0][2].squeeze(1).to(torch.uint8).to(DEV)
    cell = F_hip.pixel_contrast_labels(target, 4, (32, 32))
    assert torch.equal(cell, seen["cell_label"]) and bool((cell >= 0).all())
    want_idx, want_count = O.sample(cell.cpu().numpy(), 4, 16, 11)
    assert np.array_equal(seen["idx"].cpu().numpy(), want_idx) and np.array_equal(seen["count"].cpu().numpy(), want_count)
    idx, count = real_sample(seen["cell_label"], 4, 16, seen["word"])
    assert torch.equal(idx, seen["idx"]) and torch.equal(count, seen["count"])
    again = real_crit(ep._hooks[0], seen["feature"], idx, count).detach()
    assert torch.equal(again, seen["loss"])
    assert torch.equal(reg.detach(), 0.5 * again) and bool(torch.isfinite(reg)) and float(reg.detach()) > 0.0
    cnt = [int(v) for v in count.tolist()]
    print(f"step: counts {cnt}, loss {float(again):.6f}")
    got = ep.meters.statistics()["pixelcontrast"]
    assert got["loss"]["mean"] == pytest.approx(float(again), rel=1e-6)
    assert got["anchors"]["mean"] == pytest.approx(O.anchors(cnt) / 64.0, rel=1e-6)
    assert got["filled"]["mean"] == pytest.approx(sum(cnt) / 64.0, rel=1e-6)
    assert got["fg_filled"]["mean"] == pytest.approx(sum(cnt[1:]) / 48.0, rel=1e-6)
    assert cnt == [16, 16, 16, 16]
    ep.close_hooks()


def test_gradient_reaches_the_head_and_the_layers_up_to_the_feature():
    from spcl_amd.semi_seg.hooks import PixelContrastTrainerHook
    _, model = _unet()
    hook = PixelContrastTrainerHook(name="pixelcontrast", model=model, **PC)
    hook.to(DEV)
    eh = _drive(hook, model)
    lab = _blocky(_batch(2, 64, 1), 5)
    eh.before_forward_pass()
    model(lab[0][0].to(DEV))
    eh.after_forward_pass()
    loss = eh(labeled_target=lab[0][2].squeeze(1).to(DEV))
    loss.backward()
    torch.cuda.synchronize()
    for name, p in hook._projector.named_parameters():
        assert p.grad is not None and float(p.grad.abs().max()) > 0.0, name
    names = list(model.arch_elements)
    upto = names[:names.index("Up_conv3") + 1]
    reached, beyond = [], []
    for name, p in model.named_parameters():
        block = name.split(".")[0].lstrip("_")
        (reached if block in upto else beyond).append((name, p))
    assert reached and beyond
    for name, p in reached:
        assert p.grad is not None and bool(torch.isfinite(p.grad).all()) and float(p.grad.abs().max()) > 0.0, name
    for name, p in beyond:
        assert p.grad is None or float(p.grad.abs().max()) == 0.0, name
    eh.close()


def test_draw_advances_without_a_host_synchronisation():
    sd, model, hook, ep, flat = _setup("PixelContrastParameters", PC)
    with ep.meters.focus_on(ep.meter_focus):
        ep.step(_blocky(_batch(2, 64, 1), 5), _batch(2, 64, 2), seed=1)  # (first step: allocations, lazy initialisation)
        torch.cuda.synchronize()
        assert hook.draw.tolist() == [12]
        batches = [(_blocky(_batch(2, 64, 10 + k), 6 + k), _batch(2, 64, 20 + k)) for k in range(2)]
        moved = [tuple(((tuple(t.pin_memory() for t in b[0]),) + b[1:]) for b in pair) for pair in batches]
        for k, (lab, unl) in enumerate(moved):
            torch.cuda.set_sync_debug_mode("error")
            try:
                ep.step(lab, unl, seed=2 + k)
            finally:
                torch.cuda.set_sync_debug_mode(0)
            torch.cuda.synchronize()
            assert hook.draw.tolist() == [13 + k]
    got = ep.meters.statistics()["pixelcontrast"]
    assert got["filled"]["mean"] == pytest.approx(1.0) and got["loss"]["mean"] > 0.0
    ep.close_hooks()


def test_unlabeled_threshold_samples_cells_of_unlabelled_slices(monkeypatch):
    sd, model, hook, ep, flat = _setup("PixelContrastParameters", dict(PC, unlabeled_threshold=0.3))
    seen, _, _ = _spy(monkeypatch)
    with ep.meters.focus_on(ep.meter_focus):
        sup, reg = ep.step(_blocky(_batch(2, 64, 1), 5), _batch(2, 64, 2), seed=1234)
    torch.cuda.synchronize()
    assert tuple(seen["cell_label"].shape) == (4, 32, 32) and seen["feature"].shape[0] == 4
    idx = seen["idx"].cpu()
    unlabelled = int((idx >= 2 * 32 * 32).sum())
    print(f"threshold 0.3: {unlabelled} of {int((idx >= 0).sum())} sampled cells lie in unlabelled slices; "
          f"eligible unlabelled cells {int((seen['cell_label'][2:] >= 0).sum())}")
    assert unlabelled > 0 and bool(torch.isfinite(reg))
    ep.close_hooks()


def test_two_seeded_trainer_runs_are_identical():
    ends = []
    for _ in range(2):
        tr, model, _, _ = _trainer(_cfg(PixelContrastParameters=PC))
        random.seed(7)
        hist = tr.start_training()
        torch.cuda.synchronize()
        assert len(hist) == 2
        for name in ("pixelcontrast", "loss", "anchors", "filled", "fg_filled"):
            assert name in str(hist[-1]["tra"]), name
        hook = tr.__hooks__[0]
        ends.append((_snapshot(model), _snapshot(hook._projector), hook.draw.cpu().clone()))
    (pa, ha, da), (pb, hb, db) = ends
    assert all(torch.equal(pa[k], pb[k]) for k in pa) and all(torch.equal(ha[k], hb[k]) for k in ha)
    assert torch.equal(da, db) and da.tolist() == [11 + 6]  # two epochs of three steps


def test_trainer_round_trip_restores_draw_and_the_next_step():
    tr, model, lab, unl = _trainer(_cfg(PixelContrastParameters=PC))
    ep = tr._create_tra_epoch()
    with ep.meters.focus_on(ep.meter_focus):
        for k in range(2):
            ep.step(lab[k], unl[k], seed=100 + k)
        torch.cuda.synchronize()
        blob = io.BytesIO()
        torch.save(tr.state_dict(), blob)
        hook = tr.__hooks__[0]
        assert hook.draw.tolist() == [13]
        ep.step(lab[2], unl[2], seed=102)
    torch.cuda.synchronize()
    ep.close_hooks()
    want = (_snapshot(model), _snapshot(hook._projector), hook.draw.cpu().clone())

    blob.seek(0)
    saved = torch.load(blob, map_location="cpu")
    assert "0.draw" in saved["__hooks__"] and saved["__hooks__"]["0.draw"].dtype == torch.int32
    tr2, model2, _, _ = _trainer(_cfg(PixelContrastParameters=dict(PC, seed=99)), seed=4)  # (other weights, other seed)
    tr2.load_state_dict(saved)
    hook2 = tr2.__hooks__[0]
    assert hook2.draw.is_cuda and hook2.draw.tolist() == [13]
    ep2 = tr2._create_tra_epoch()
    with ep2.meters.focus_on(ep2.meter_focus):
        ep2.step(lab[2], unl[2], seed=102)
    torch.cuda.synchronize()
    ep2.close_hooks()
    got, head = _snapshot(model2), _snapshot(hook2._projector)
    assert torch.equal(hook2.draw.cpu(), want[2]) and want[2].tolist() == [14]
    assert all(torch.equal(got[k], want[0][k]) for k in got) and all(torch.equal(head[k], want[1][k]) for k in head)


def test_without_the_section_the_trainer_is_what_it_was(monkeypatch):
    from spcl_amd.semi_seg.epochers.semi import SemiSupervisedEpocher
    from spcl_amd.semi_seg.hooks import MeanTeacherTrainerHook, PixelContrastTrainerHook
    none, _, _, _ = _trainer(_cfg())
    both, _, _, _ = _trainer(_cfg(MeanTeacherParameters=MT, PixelContrastParameters=PC))
    assert [type(h) for h in none.__hooks__] == []
    assert [type(h) for h in both.__hooks__] == [MeanTeacherTrainerHook, PixelContrastTrainerHook]

    def meter_names(tr):
        ep = tr._create_tra_epoch()
        names = {g: sorted(ms) for g, ms in ep.meters._groups.items()}
        ep.close_hooks()
        return names

    base = meter_names(none)
    assert sorted(base) == ["semi"] and base["semi"] == ["lr", "reg_loss", "sup_dice", "sup_loss"]
    assert meter_names(both) == dict(base, meanteacher=["loss"], pixelcontrast=["anchors", "fg_filled", "filled", "loss"])

    def three_steps(strip):
        """a mean-teacher trainer's first three steps; ``strip`` drops the two keywords nobody but the new hook reads"""
        tr, model, lab, unl = _trainer(_cfg(MeanTeacherParameters=MT))
        assert all("draw" not in k for k in tr.__hooks__.state_dict())
        ep = tr._create_tra_epoch()
        if strip:
            real = SemiSupervisedEpocher._regularization

            def without(self, **kwargs):
                assert "labeled_target" in kwargs and "label_logits" in kwargs
                kwargs.pop("labeled_target")
                kwargs.pop("label_logits")
                return real(self, **kwargs)

            monkeypatch.setattr(SemiSupervisedEpocher, "_regularization", without)
        out = []
        with ep.meters.focus_on(ep.meter_focus):
            for k in range(3):
                sup, reg = ep.step(lab[k], unl[k], seed=50 + k)
                out.append((sup.detach().cpu().clone(), reg.detach().cpu().clone()))
        torch.cuda.synchronize()
        ep.close_hooks()
        if strip:
            monkeypatch.undo()
        return out, _snapshot(model)

    (la, pa), (lb, pb) = three_steps(False), three_steps(True)
    assert all(torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) for a, b in zip(la, lb))
    assert all(torch.equal(pa[k], pb[k]) for k in pa)


def test_a_label_batch_of_one_class_gives_zero_and_a_finite_step():
    sd, model, hook, ep, flat = _setup("PixelContrastParameters", PC)
    (img, img_tf, tgt, _), names, groups = _batch(2, 64, 1)
    one = torch.full_like(tgt, 2)
    before = _snapshot(model)
    with ep.meters.focus_on(ep.meter_focus):
        sup, reg = ep.step(((img, img_tf, one, one.clone()), names, groups), _batch(2, 64, 2), seed=3)
    torch.cuda.synchronize()
    # (the sample holds class 2 alone: positives without negatives, which the hook answers with an exact zero)
    assert float(reg.detach()) == 0.0 and bool(torch.isfinite(sup))
    assert ep.meters.statistics()["pixelcontrast"]["filled"]["mean"] == pytest.approx(0.25)
    after = _snapshot(model)
    assert all(bool(torch.isfinite(after[k]).all()) for k in after)
    assert any(not torch.equal(after[k], before[k]) for k in before)
    ep.close_hooks()
