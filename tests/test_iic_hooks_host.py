"""CPU: the UDA-IIC section of the config (config/hooks/udaiic.yaml) builds the reference's hook set through
``hook_creator.create_hook_from_config``: names, state_dict keys, the cluster heads' initial weights under one seed, the
``ntuple`` handling of weights and paddings; pre-training still refuses it.  The float64 helper's dense criterion agrees
with its joint-level restatement."""
import pytest
import torch
from torch import nn

from tests import _iic_oracle as R

UDAIIC = {"feature_names": ["Conv5", "Up_conv3", "Up_conv2"], "mi_weights": [0.1, 0.05, 0.05], "dense_paddings": None,
          "consistency_weight": 1}


def _config(**over):
    return {"Data": {"name": "acdc"}, "Trainer": {"max_epoch": 2}, "DiscreteMIConsistencyParams": dict(UDAIIC, **over)}


def _model():
    from spcl_amd.semi_seg.arch import UNet
    return UNet(input_dim=1, num_classes=4, max_channel=256)


def _build(**over):
    from spcl_amd.hook_creator import create_hook_from_config
    model = _model()
    torch.manual_seed(5)
    hooks = create_hook_from_config(model, _config(**over), is_pretrain=False)
    assert len(hooks) == 1
    return hooks[0]


def test_udaiic_hook_set_names_and_criteria():
    from spcl_amd.contrastyou.losses.iic_loss import IIDLoss, IIDSegmentationLoss
    hook = _build()
    mi, cons = hook._hooks
    assert [h._hook_name for h in mi._hooks] == ["discreteMI/conv5", "discreteMI/up_conv3", "discreteMI/up_conv2"]
    assert cons._hook_name == "consistency" and cons._weight == 1
    assert [h._weight for h in mi._hooks] == [0.1, 0.05, 0.05]
    assert isinstance(mi._hooks[0]._criterion, IIDLoss)
    assert [type(h._criterion) for h in mi._hooks[1:]] == [IIDSegmentationLoss] * 2
    assert [h._criterion.padding for h in mi._hooks[1:]] == [0, 0]


def test_udaiic_state_dict_keys_and_initial_weights():
    hook = _build()
    sd = hook.state_dict()
    keys = []
    for h, (kind, idx) in enumerate([("lin", 2), ("conv", 0), ("conv", 0)]):
        for s in range(5):
            keys += [f"_hooks.0._hooks.{h}._projector._headers.{s}.{idx}.weight",
                     f"_hooks.0._hooks.{h}._projector._headers.{s}.{idx}.bias"]
    assert sorted(sd) == sorted(keys)
    # the reference's construction order under the same seed: 5 x Linear(256, 20), 5 x Conv2d(32, 20, 1), 5 x Conv2d(16, 20, 1)
    torch.manual_seed(5)
    ref = [nn.Linear(256, 20) for _ in range(5)] + [nn.Conv2d(32, 20, 1) for _ in range(5)] + \
          [nn.Conv2d(16, 20, 1) for _ in range(5)]
    for n, m in enumerate(ref):
        h, s = divmod(n, 5)
        idx = 2 if h == 0 else 0
        assert torch.equal(sd[f"_hooks.0._hooks.{h}._projector._headers.{s}.{idx}.weight"], m.weight.detach())
        assert torch.equal(sd[f"_hooks.0._hooks.{h}._projector._headers.{s}.{idx}.bias"], m.bias.detach())


def test_ntuple_cases():
    hook = _build(mi_weights=0.2, dense_paddings=[0, 1])
    mi = hook._hooks[0]
    assert [h._weight for h in mi._hooks] == [0.2, 0.2, 0.2]
    assert [h._criterion.padding for h in mi._hooks[1:]] == [0, 1]
    hook = _build(dense_paddings=[3])
    assert [h._criterion.padding for h in hook._hooks[0]._hooks[1:]] == [3, 3]
    with pytest.raises(RuntimeError):
        _build(dense_paddings=[0, 1, 3])


def test_pretrain_still_refuses_the_section():
    from spcl_amd.hook_creator import create_hook_from_config
    with pytest.raises(RuntimeError):
        create_hook_from_config(_model(), _config(), is_pretrain=True)


def test_install_aliases_the_new_modules():
    import spcl_amd
    spcl_amd.install()
    from semi_seg.hooks.discretemi import DiscreteMITrainHook  # noqa: F401
    from semi_seg.hooks.consistency import ConsistencyTrainerHook  # noqa: F401
    from contrastyou.losses.iic_loss import IIDLoss, IIDSegmentationLoss  # noqa: F401
    from semi_seg.hooks import create_discrete_mi_consistency_hook  # noqa: F401


@pytest.mark.parametrize("pad", [0, 1, 3])
def test_oracle_dense_criterion_restatements_agree(pad):
    g = torch.Generator().manual_seed(pad)
    px = torch.randn(2, 20, 9, 13, generator=g, dtype=torch.float64).softmax(1)
    py = torch.randn(2, 20, 9, 13, generator=g, dtype=torch.float64).softmax(1)
    a = R.iid_segmentation_loss(px, py, pad)
    b = R.dense_loss_from_joint(R.joint_dense(px, py, pad))
    assert abs(float(a) - float(b)) <= 1e-12 * abs(float(a))


def test_main_import_line_resolves_after_install():
    """reference main.py:15 imports the three trainers from new_trainer; MixUpTrainer is a stub that refuses construction"""
    import spcl_amd
    spcl_amd.install()
    from semi_seg.trainers.new_trainer import SemiTrainer, FineTuneTrainer, MixUpTrainer  # noqa: F401
    from semi_seg.epochers.new_epocher import SemiSupervisedEpocher  # noqa: F401
    assert issubclass(SemiTrainer, FineTuneTrainer)
    with pytest.raises(NotImplementedError):
        MixUpTrainer()


def test_flip_flags_must_live_on_the_device():
    from spcl_amd import functional as F_hip
    with pytest.raises(RuntimeError):
        F_hip._flip_flags_arg(torch.tensor([1, 2], dtype=torch.uint8), 2, torch.device("cpu"))
