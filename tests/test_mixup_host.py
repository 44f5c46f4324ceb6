"""CPU: the host side of the mix-up baseline.  The hook's draws under a seed are the reference's (``np.random.beta`` then
``torch.randperm`` after seeding python, numpy and torch) and leave the three generators as they found them; ``MixupPlan``
refuses what the kernels must not index by and keeps the f32 pair torch would compute with; after ``install()`` the
reference's import lines resolve; ``MixUpTrainer`` builds on the CPU; the two launches have no CPU path."""
import random

import numpy as np
import pytest
import torch

from tests import _mixup_oracle as M


@pytest.mark.parametrize("batch", [1, 2, 5])
@pytest.mark.parametrize("seed", [0, 1234, 9999999])
def test_draws_are_the_references_and_restore_the_generators(seed, batch):
    from spcl_amd.semi_seg.hooks.mixup import mixup_draw
    random.seed(7)
    np.random.seed(8)
    torch.manual_seed(9)
    before = random.getstate(), np.random.get_state(), torch.get_rng_state()
    lam, index = mixup_draw(seed, 2 * batch)
    after = random.getstate(), np.random.get_state(), torch.get_rng_state()
    assert before[0] == after[0]
    assert before[1][0] == after[1][0] and np.array_equal(before[1][1], after[1][1]) and before[1][2:] == after[1][2:]
    assert torch.equal(before[2], after[2])
    # the restated draw, computed here: randperm's stream belongs to the installed torch
    random.seed(seed)
    np.random.seed(seed)
    torch.manual_seed(seed)
    want_lam = np.random.beta(1, 1)
    want_index = torch.randperm(2 * batch)
    assert lam == want_lam and 0.0 <= lam <= 1.0
    assert torch.equal(index, want_index)
    olam, oindex = M.draw(seed, 2 * batch)
    assert olam == want_lam and torch.equal(oindex, want_index)


def test_fix_all_seed_leaves_fix_random_seed_alone():
    from spcl_amd.semi_seg.epochers.helper import FixAllSeed, FixRandomSeed
    torch.manual_seed(3)
    state = torch.get_rng_state()
    with FixRandomSeed(5):
        a = random.random()
    assert torch.equal(torch.get_rng_state(), state)  # (seeds python and numpy only, as before)
    with FixAllSeed(5):
        b = random.random()
        t = torch.rand(1)
    torch.manual_seed(5)
    assert a == b and torch.equal(t, torch.rand(1))


def test_mixup_plan_checks_the_permutation():
    from spcl_amd.functional import MixupPlan
    for bad in ([0, 1, 2], [0, 1, 2, -1], [0, 1, 2, 4], torch.tensor([1, 0, 4, 2]), torch.tensor([0, 1, 2]), []):
        with pytest.raises(ValueError):
            MixupPlan(bad, 0.3, "cpu")
    with pytest.raises(ValueError):
        MixupPlan(torch.tensor([0.0, 1.0]), 0.3, "cpu")
    for lam in (0.23538938957272115, 1.0, 3.7816489242002753e-4, np.float64(0.7431448254773942)):
        perm = torch.randperm(6)
        plan = MixupPlan(perm, lam, "cpu")
        assert plan.n2 == 6 and plan.lam == lam
        assert plan.index.dtype == torch.int32 and plan.index.tolist() == perm.tolist()
        want = torch.tensor(lam, dtype=torch.float32), torch.tensor(1 - lam, dtype=torch.float32)
        assert plan.pair == (float(want[0]), float(want[1]))
        assert torch.tensor(plan.pair[0], dtype=torch.float32) == want[0]
        assert torch.tensor(plan.pair[1], dtype=torch.float32) == want[1]
    assert MixupPlan([1, 0], 0.5, "cpu").index.tolist() == [1, 0]


def test_reference_import_lines_resolve_after_install():
    import spcl_amd
    spcl_amd.install()
    from semi_seg.hooks.mixup import MixUpHook
    from semi_seg.epochers.new_comparable import MixUpEpocher
    from semi_seg.trainers.new_trainer import MixUpTrainer
    from semi_seg.epochers.new_epocher import SemiSupervisedEpocher
    from semi_seg.hooks import MixUpHook as exported
    assert exported is MixUpHook and issubclass(MixUpEpocher, SemiSupervisedEpocher)
    assert MixUpTrainer.train_epocher.fget(None) is MixUpEpocher
    # main_mixup.py:61 with config/base.yaml's section
    hook = MixUpHook(hook_name="mx_hook_host_test", **{"weight": 0.01, "enable_bn": True})
    eh = hook()
    assert eh._name == "mix_reg" and eh._weight == 0.01 and eh._enable_bn is True
    assert list(hook.parameters()) == []


def test_mixup_trainer_builds_on_the_cpu():
    from spcl_amd.contrastyou.losses.kl import KL_div
    from spcl_amd.semi_seg.arch import UNet
    from spcl_amd.semi_seg.epochers.mixup import MixUpEpocher
    from spcl_amd.semi_seg.trainers.semi import MixUpTrainer, SemiTrainer
    model = UNet(input_dim=1, num_classes=4, max_channel=128)
    tr = MixUpTrainer(model=model, labeled_loader=[], unlabeled_loader=[], val_loader=[], test_loader=None,
                      criterion=KL_div(), save_dir=None, max_epoch=1, num_batches=1, device="cpu")
    assert isinstance(tr, SemiTrainer) and tr.train_epocher is MixUpEpocher and tr.activate_hooks
    with pytest.raises(NotImplementedError):
        MixUpTrainer()


def test_epocher_refuses_a_loader_without_total_freedom():
    import types
    from spcl_amd.contrastyou.losses.kl import KL_div
    from spcl_amd.semi_seg.arch import UNet
    from spcl_amd.semi_seg.epochers.mixup import MixUpEpocher
    model = UNet(input_dim=1, num_classes=4, max_channel=128)
    opt = torch.optim.SGD(model.parameters(), lr=0.0)

    def build(loader):
        return MixUpEpocher(model=model, optimizer=opt, labeled_loader=loader, unlabeled_loader=None,
                            sup_criterion=KL_div(), num_batches=1, device="cpu")

    build([]).init()
    build(types.SimpleNamespace(_total_freedom=True)).init()
    with pytest.raises(AssertionError):
        build(types.SimpleNamespace(_total_freedom=False)).init()


def test_the_launches_have_no_cpu_path():
    from spcl_amd import functional as F_hip
    plan = F_hip.MixupPlan([1, 0, 3, 2], 0.4, "cpu")
    img = torch.rand(2, 1, 8, 8)
    tgt = torch.randint(0, 4, (2, 1, 8, 8))
    with pytest.raises(RuntimeError, match="MI355X"):
        F_hip.mixup_images(img, img, plan)
    with pytest.raises(RuntimeError, match="MI355X"):
        F_hip.mixup_kl_onehot(torch.randn(4, 4, 8, 8), tgt, tgt, plan)


def test_oracle_mixed_target_is_a_simplex_and_agrees_with_the_f32_formulation():
    """the restated ``mixed_y`` against the reference's own f32 expression on int64 one-hot maps (mixup.py:31,66-71)"""
    g = torch.Generator().manual_seed(4)
    tgt, tgt_tf = torch.randint(0, 4, (3, 1, 9, 7), generator=g), torch.randint(0, 4, (3, 1, 9, 7), generator=g)
    lam, index = M.draw(11, 6)
    y64 = M.mixed_y(tgt, tgt_tf, lam, index, 4)
    assert torch.allclose(y64.sum(1), torch.ones(6, 9, 7, dtype=torch.float64), atol=1e-15)
    oh = torch.nn.functional.one_hot(torch.cat([tgt, tgt_tf]).squeeze(1), 4).permute(0, 3, 1, 2)
    y32 = lam * oh + (1 - lam) * oh[index, :]
    assert y32.dtype == torch.float32 and float((y32.double() - y64).abs().max()) <= 2.0 ** -23
