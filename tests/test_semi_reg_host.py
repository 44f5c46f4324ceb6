"""CPU: the mean-teacher and entropy-minimisation baselines are wired in -- the reference's import lines resolve after
``install()``, ``create_hook_from_config`` builds each hook from its config section (``MeanTeacherParameters`` as in
config/specific/mt.yaml, ``EntropyMinParameters``) and refuses both during pre-training, the teacher is a detached copy
that the trainer's optimizer cannot reach -- and the two restated deepclustering2 pieces (``EMAUpdater``'s ramped alpha,
``Entropy``) follow their definitions."""
import pytest
import torch

MT = {"name": "mse", "weight": 10, "alpha": 0.999, "weight_decay": 0.000001}


def _config(**sections):
    return dict({"Data": {"name": "acdc"}, "Trainer": {"max_epoch": 2}}, **sections)


def _model():
    from spcl_amd.semi_seg.arch import UNet
    return UNet(input_dim=1, num_classes=4, max_channel=128)


def test_install_aliases_the_two_hook_modules():
    import spcl_amd
    done = spcl_amd.install()
    assert "semi_seg.hooks.mt" in done and "semi_seg.hooks.entmin" in done
    from semi_seg.hooks.mt import MeanTeacherTrainerHook
    from semi_seg.hooks.entmin import EntropyMinTrainerHook
    from semi_seg.hooks import MeanTeacherTrainerHook as A, EntropyMinTrainerHook as B
    from semi_seg.hooks import create_entropy_min_hook, create_mean_teacher_hook  # noqa: F401
    assert A is MeanTeacherTrainerHook and B is EntropyMinTrainerHook


def test_config_sections_build_the_hooks():
    from spcl_amd.hook_creator import create_hook_from_config
    from spcl_amd.semi_seg.hooks import EntropyMinTrainerHook, MeanTeacherTrainerHook
    model = _model()
    (mt,) = create_hook_from_config(model, _config(MeanTeacherParameters=MT))
    assert isinstance(mt, MeanTeacherTrainerHook) and mt._hook_name == "meanteacher" and mt._weight == 10
    assert mt._updater.alpha == 0.999 and mt._updater.weight_decay == 0.000001 and mt._updater.justify_alpha
    assert mt._teacher_softmax is False  # mt.py:49-52: the teacher's raw output enters the criterion
    (ent,) = create_hook_from_config(model, _config(EntropyMinParameters={"weight": 0.5}))
    assert isinstance(ent, EntropyMinTrainerHook) and ent._hook_name == "entropy" and ent._weight == 0.5
    both = create_hook_from_config(model, _config(MeanTeacherParameters=MT, EntropyMinParameters={"weight": 0.5}))
    assert [type(h) for h in both] == [MeanTeacherTrainerHook, EntropyMinTrainerHook]
    assert create_hook_from_config(model, _config()) == []


@pytest.mark.parametrize("section,params", [("MeanTeacherParameters", MT), ("EntropyMinParameters", {"weight": 0.5})])
def test_pretrain_refuses_the_sections(section, params):
    from spcl_amd.hook_creator import create_hook_from_config
    with pytest.raises(RuntimeError):
        create_hook_from_config(_model(), _config(**{section: params}), is_pretrain=True)


def test_only_the_mse_teacher_criterion_is_mirrored():
    from spcl_amd.semi_seg.hooks import create_mean_teacher_hook
    with pytest.raises(NotImplementedError):
        create_mean_teacher_hook(model=_model(), weight=1.0, name="kl")


def test_teacher_is_a_detached_copy():
    from spcl_amd.semi_seg.hooks import create_mean_teacher_hook
    model = _model()
    model.__dict__["_spcl_eval_graphs"] = object()  # what the evaluation epocher leaves on a model: must not be copied
    hook = create_mean_teacher_hook(model=model, weight=1.0)
    teacher = hook.teacher_model
    assert "_spcl_eval_graphs" in model.__dict__ and "_spcl_eval_graphs" not in teacher.__dict__
    assert teacher is not model and teacher.training == model.training
    mine = {p.untyped_storage().data_ptr() for p in model.parameters()}
    names = [k for k, _ in model.named_parameters()]
    assert [k for k, _ in teacher.named_parameters()] == names
    for (k, t), s in zip(teacher.named_parameters(), model.parameters()):
        assert not t.requires_grad and t.grad_fn is None, k
        assert t.untyped_storage().data_ptr() not in mine, k
        assert torch.equal(t, s), k
    # the teacher travels with the hook's state, but no trainable parameter of the hook exists
    assert sorted(hook.state_dict()) == sorted("_teacher_model." + k for k in model.state_dict())
    assert [p for p in hook.parameters() if p.requires_grad] == []
    model.eval()
    assert create_mean_teacher_hook(model=model, weight=1.0).teacher_model.training is False


def test_semi_trainer_keeps_the_teacher_out_of_the_optimizer(tmp_path):
    from spcl_amd.contrastyou.hooks.base import CombineTrainerHook
    from spcl_amd.contrastyou.losses.kl import KL_div
    from spcl_amd.hook_creator import create_hook_from_config
    from spcl_amd.semi_seg.trainers.semi import SemiTrainer
    model = _model()
    cfg = _config(MeanTeacherParameters=MT, Optim={"name": "SGD", "lr": 1e-5, "weight_decay": 1e-5})
    tr = SemiTrainer(model=model, labeled_loader=[], unlabeled_loader=[], val_loader=[], test_loader=None, criterion=KL_div(),
                     save_dir=str(tmp_path), max_epoch=1, num_batches=1, device="cpu", config=cfg)
    # inside a combined hook the teacher's parameters are reachable through ``parameters()``: only requires_grad keeps them out
    tr.register_hooks(CombineTrainerHook(*create_hook_from_config(model, cfg)))
    tr.init()
    n_model = sum(p.numel() for p in model.parameters())
    assert tr._flat.numel == n_model
    inside = {id(p) for p in tr._flat.params}
    teacher = tr.__hooks__[0]._hooks[0].teacher_model
    assert all(id(p) not in inside for p in teacher.parameters())
    assert any(k.endswith("_teacher_model._Conv1.conv.0.weight") for k in tr.state_dict()["__hooks__"])


def test_ema_updater_alpha_ramp():
    from spcl_amd.contrastyou.ema import EMAUpdater
    u = EMAUpdater(alpha=0.999)
    assert (u.justify_alpha, u.weight_decay, u.step) == (True, 1e-5, 0)
    got = []
    for step in (0, 1, 2, 3, 10 ** 4):
        u.step = step
        got.append(u.alpha_t)
    assert got == [0, 1 - 1 / 2, 1 - 1 / 3, 1 - 1 / 4, 0.999]
    assert got[1:4] == pytest.approx([1 / 2, 2 / 3, 3 / 4], rel=1e-15)
    v = EMAUpdater(alpha=0.99, justify_alpha=False)
    assert v.alpha_t == 0.99
    with pytest.raises(NotImplementedError):
        EMAUpdater(update_bn=True)


def test_entropy_follows_its_definition():
    import spcl_amd
    from spcl_amd.contrastyou.losses.kl import Entropy
    g = torch.Generator().manual_seed(3)
    prob = torch.randn(3, 4, 5, 6, generator=g, dtype=torch.float64).softmax(1)
    ref = -(prob * (prob + 1e-16).log()).sum(1).mean()
    assert float(Entropy()(prob)) == pytest.approx(float(ref), rel=1e-14)
    ref32 = -(prob.float() * (prob.float() + 1e-16).log()).sum(1).mean()
    assert float(Entropy(eps=1e-16)(prob.float())) == pytest.approx(float(ref), rel=1e-6)
    assert torch.equal(Entropy()(prob.float()), ref32)
    with pytest.raises(AssertionError):
        Entropy()(prob * 1.5)
    assert float(Entropy()(prob * 1.5, disable_assert=True)) > 0
    with pytest.raises(NotImplementedError):
        Entropy(reduction="sum")
    spcl_amd.install()
    from deepclustering2.loss import Entropy as E2  # noqa: F401  (the mirror's, or the real package where it is installed)
