"""GPU: the uncertainty-aware mean-teacher hook (semi_seg/hooks/ucmt.py).

Replay: the student and its teacher are in ``eval()`` (stateless forwards).  The test seeds torch's device generator, rebuilds
the hook's noise sequence from the same seed, runs a COPY of the teacher (taken before the call) on it -- for both
``cumulative_noise`` settings -- and restates the criterion in float64 on those maps (tests/_ucmt_oracle.py).  The threshold
is the median of that float64 entropy, so that the mask is neither empty nor full.  The mask rule is the one of
tests/test_gpu_ucmt_kernels.py: the kernel's mask (taken from the hook's own call of ``functional.ucmt_softmax_mse``) equals
the oracle's outside a band of 2e-6 around the threshold, the band holds at most max(1, 0.2 % of M) pixels (asserted on the
oracle alone), and loss and student-logit gradient are within 1e-5 of the oracle evaluated with the kernel's mask.

Also: the caller's image is untouched, the teacher moved by the moving-average formula (the bound of
tests/test_gpu_semi_reg_hooks.py), the BatchNorm tracking flags of the student are unchanged and the teacher's restored,
the meters hold the threshold and kept / M, a second epoch sees the stepped threshold, and one ``SemiSupervisedEpocher``
step with the hook registered runs and moves student and teacher."""
import pytest
import torch

from tests import _ucmt_oracle as UO
from tests.test_gpu_semi_reg_hooks import _drive, _ema_check, _setup, _snapshot, _unet
from tests.test_gpu_semi_step import _batch, _rel_l2

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
BAND = 2e-6
SEED = 4321
UC = {"name": "mse", "weight": 10, "alpha": 0.999, "weight_decay": 0.000001}


class _Steps:
    """a threshold schedule with given values"""

    def __init__(self, *values):
        self.values, self.epoch = values, 0

    value = property(lambda self: self.values[min(self.epoch, len(self.values) - 1)])

    def step(self):
        self.epoch += 1


def _track_flags(module):
    return [m.track_running_stats for m in module.modules() if hasattr(m, "track_running_stats")]


def _replay(replica, img, num_samples, noise_std, cumulative):
    """what the hook computes, on a copy of the teacher: the clean map and the noisy ones from the seeded noise sequence"""
    from spcl_amd.semi_seg.hooks.ucmt import bn_track_off
    torch.cuda.manual_seed(SEED)
    with torch.no_grad():
        clean = replica(img).float().cpu()
        noises = [noise_std * torch.randn_like(img) for _ in range(num_samples)]
        noisy, acc = [], img.clone()
        with bn_track_off(replica):
            for z in noises:
                if cumulative:
                    acc = acc + z
                    noisy.append(replica(acc).float().cpu())
                else:
                    noisy.append(replica(img + z).float().cpu())
    return clean, noisy


@pytest.mark.parametrize("cumulative", [True, False])
def test_uc_mean_teacher_hook_replays_against_float64(cumulative, monkeypatch):
    from spcl_amd import functional as F_hip
    from spcl_amd.semi_seg.hooks.mt import _copy_model
    from spcl_amd.semi_seg.hooks.ucmt import UCMeanTeacherTrainerHook
    _, model = _unet()
    model.eval()
    schedule = _Steps(0.0, 0.5)
    th = UCMeanTeacherTrainerHook("ucmeanteacher", 10.0, model, max_epoch=30, alpha=0.999, weight_decay=1e-5,
                                  threshold=schedule, cumulative_noise=cumulative)
    th.to(DEV)
    assert th.teacher_model.training is False
    with torch.no_grad():  # a student that has moved away from its teacher
        g = torch.Generator().manual_seed(5)
        for p in model.parameters():
            p.add_(0.05 * torch.randn(p.shape, generator=g).to(DEV))
    th._updater.step = 3  # alpha_t = 3/4
    g = torch.Generator().manual_seed(1)
    img = torch.rand(3, 1, 32, 32, generator=g).to(DEV)
    b = torch.randn(3, 4, 32, 32, generator=g)
    flags = [3, 0, 1]
    replica = _copy_model(th.teacher_model)
    clean, noisy = _replay(replica, img, 8, 0.05, cumulative)
    u64 = UO.entropy(noisy, flags)
    M = u64.numel()
    value = float(u64.flatten().median().float())  # an f32 value: what the kernel is handed
    schedule.values = (value, 0.5)
    in_band = (u64 - value).abs() <= BAND
    print(f"entropy {float(u64.min()):.6f} .. {float(u64.max()):.6f}, threshold {value:.6f}, in band {int(in_band.sum())}")
    assert int(in_band.sum()) <= max(1, int(0.002 * M)), int(in_band.sum())

    seen = {}
    real = F_hip.ucmt_softmax_mse

    def spy(teacher, noisy_list, student_logits, threshold, *args, **kwargs):
        loss = real(teacher, noisy_list, student_logits, threshold, *args, **kwargs)
        seen.update(teacher=teacher, noisy=list(noisy_list), threshold=threshold, out=kwargs["out"])
        return loss

    monkeypatch.setattr(F_hip, "ucmt_softmax_mse", spy)
    eh = _drive(th, model)
    assert schedule.epoch == 1  # read, then stepped, in the trainer hook's __call__
    before, student = _snapshot(th.teacher_model), _snapshot(model)
    flags_student, flags_teacher = _track_flags(model), _track_flags(th.teacher_model)
    img_before = img.clone()
    bd = b.to(DEV).contiguous(memory_format=torch.channels_last).requires_grad_(True)
    torch.cuda.manual_seed(SEED)
    loss = eh(unlabeled_tf_logits=bd, unlabeled_image=img, seed=0, affine_transformer=None,
              flip_flags=torch.tensor(flags, dtype=torch.uint8, device=DEV))
    loss.backward()
    assert torch.equal(img, img_before)
    assert _track_flags(model) == flags_student and _track_flags(th.teacher_model) == flags_teacher
    assert all(flags_teacher)
    # the maps the hook handed to the kernel are the replayed ones
    assert seen["threshold"] == value and len(seen["noisy"]) == 8
    assert _rel_l2(seen["teacher"], clean) <= 1e-6
    for got, want in zip(seen["noisy"], noisy):
        assert _rel_l2(got, want) <= 1e-6
    kept, mask = seen["out"]
    mask = mask.cpu()
    wrong = (mask.bool() != (u64 <= value)) & ~in_band
    assert int(wrong.sum()) == 0, int(wrong.sum())
    assert int(kept) == int(mask.sum()) and 0 < int(kept) < M
    b64 = b.double().requires_grad_(True)
    ref = 10.0 * UO.loss(clean, b64, mask, 1.0, flags)
    ref.backward()
    lerr = abs(float(loss.detach()) - float(ref.detach())) / float(ref.detach())
    gerr = _rel_l2(bd.grad, b64.grad)
    print(f"cumulative={cumulative}: kept {int(kept)} of {M}, loss rel {lerr:.2e}, grad rel L2 {gerr:.2e}")
    assert lerr <= 1e-5 and gerr <= 1e-5, (lerr, gerr)
    # the moving average ran in this call, on a flat teacher
    assert th._updater.step == 4
    _ema_check(_snapshot(th.teacher_model), before, student, 0.75, 1e-5)
    assert len({p.untyped_storage().data_ptr() for p in th.teacher_model.parameters()}) == 1
    # meters
    stats = eh.meters.statistics()["ucmeanteacher"]
    assert stats["uc_weight"]["mean"] == pytest.approx(value, rel=1e-12)
    assert stats["uc_ratio"]["mean"] == pytest.approx(int(kept) / M, rel=1e-6)
    assert stats["loss"]["mean"] == pytest.approx(float(loss.detach()) / 10.0, rel=1e-6)
    # a second epoch sees the stepped threshold
    eh2 = _drive(th, model)
    assert eh2._threshold == 0.5 and schedule.epoch == 2
    eh2(unlabeled_tf_logits=bd, unlabeled_image=img, seed=0, affine_transformer=None,
        flip_flags=torch.tensor(flags, dtype=torch.uint8, device=DEV))
    assert seen["threshold"] == 0.5
    assert eh2.meters.statistics()["ucmeanteacher"]["uc_weight"]["mean"] == 0.5


def test_semi_step_with_the_uc_mean_teacher():
    from spcl_amd.semi_seg.hooks.ucmt import UCMeanTeacherTrainerHook
    sd, model, hook, ep, flat = _setup("UCMeanTeacherParameters", dict(UC, num_samples=2))
    assert isinstance(hook, UCMeanTeacherTrainerHook)
    lab, unl = _batch(2, 64, 1), _batch(2, 64, 2)
    teacher = hook.teacher_model
    inside = {id(p) for p in flat.params}
    assert all(id(p) not in inside and not p.requires_grad for p in teacher.parameters())
    with torch.no_grad():
        g = torch.Generator().manual_seed(5)
        for p in model.parameters():
            p.add_(0.05 * torch.randn(p.shape, generator=g).to(DEV))
    hook._updater.step = 3
    t_before, s_before = _snapshot(teacher), _snapshot(model)
    flags_student, flags_teacher = _track_flags(model), _track_flags(teacher)
    torch.cuda.manual_seed(SEED)
    with ep.meters.focus_on(ep.meter_focus):
        sup, reg = ep.step(lab, unl, seed=1234)
    torch.cuda.synchronize()
    s_after = _snapshot(model)
    assert any(not torch.equal(s_after[k], s_before[k]) for k in s_before)  # (the optimizer did step)
    assert bool(torch.isfinite(sup)) and bool(torch.isfinite(reg)) and float(reg) >= 0.0
    _ema_check(_snapshot(teacher), t_before, s_before, 0.75, UC["weight_decay"])  # (the student's weights from BEFORE the step)
    assert hook._updater.step == 4
    assert _track_flags(model) == flags_student and _track_flags(teacher) == flags_teacher
    stats = ep.meters.statistics()["ucmeanteacher"]
    assert stats["uc_weight"]["mean"] == 1.0  # max_epoch 2: RampScheduler(0, 0, ...) is at its maximum
    assert 0.0 <= stats["uc_ratio"]["mean"] <= 1.0
    ep.close_hooks()
