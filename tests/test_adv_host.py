"""CPU-only: the adversarial baseline's host side -- the reference's import names after ``install()``, the discriminator's
``state_dict`` layout and seeded initialisation, the refusal of CPU tensors, the trainer's construction."""
import pytest
import torch

# semi_seg/arch/discr.py:17-36 as an nn.Sequential: 5 convolutions without bias, 3 BatchNorm2d (hidden_dim = 64, input 4)
REFERENCE_STATE = [
    ("_main.0.weight", (64, 4, 4, 4)),
    ("_main.2.weight", (128, 64, 4, 4)),
    ("_main.3.weight", (128,)), ("_main.3.bias", (128,)), ("_main.3.running_mean", (128,)), ("_main.3.running_var", (128,)),
    ("_main.3.num_batches_tracked", ()),
    ("_main.5.weight", (256, 128, 4, 4)),
    ("_main.6.weight", (256,)), ("_main.6.bias", (256,)), ("_main.6.running_mean", (256,)), ("_main.6.running_var", (256,)),
    ("_main.6.num_batches_tracked", ()),
    ("_main.8.weight", (512, 256, 4, 4)),
    ("_main.9.weight", (512,)), ("_main.9.bias", (512,)), ("_main.9.running_mean", (512,)), ("_main.9.running_var", (512,)),
    ("_main.9.num_batches_tracked", ()),
    ("_main.11.weight", (1, 512, 4, 4)),
]


def test_reference_names_resolve_after_install():
    import spcl_amd
    spcl_amd.install()
    import semi_seg.arch.discr as discr
    from semi_seg.epochers.new_comparable import AdversarialEpocher
    from semi_seg.epochers.new_epocher import SemiSupervisedEpocher
    # main_adv.py:5-13, the lines whose modules this package mirrors (loguru, contrastyou.configure and contrastyou.utils come
    # from the reference checkout / site-packages, as for the other drivers)
    from deepclustering2.loss import KL_div  # noqa: F401
    from contrastyou import success  # noqa: F401
    from semi_seg.arch import UNet  # noqa: F401
    from semi_seg.data.creator import get_data  # noqa: F401
    from semi_seg.trainers.new_trainer import SemiTrainer, AdversarialTrainer
    assert issubclass(AdversarialEpocher, SemiSupervisedEpocher) and issubclass(AdversarialTrainer, SemiTrainer)
    assert AdversarialTrainer.train_epocher.fget(None) is AdversarialEpocher and AdversarialTrainer.activate_hooks is False
    assert hasattr(discr, "Discriminator") and hasattr(discr, "weights_init")


def test_discriminator_state_dict_is_the_references():
    from spcl_amd.semi_seg.arch.discr import Discriminator
    sd = Discriminator(4, 64).state_dict()
    assert [(k, tuple(v.shape)) for k, v in sd.items()] == REFERENCE_STATE
    assert all(v.dtype == (torch.int64 if k.endswith("num_batches_tracked") else torch.float32) for k, v in sd.items())
    # a checkpoint written by the plain torch formulation loads strictly
    from tests import _adv_oracle as A
    ref = A.discriminator(5, 8, torch.float32)
    Discriminator(5, 8).load_state_dict({"_main." + k: v for k, v in ref.state_dict().items()}, strict=True)


def test_initialisation_is_seeded_and_dcgan():
    from spcl_amd.semi_seg.arch.discr import Discriminator
    torch.manual_seed(10)
    a = Discriminator(4, 64)
    torch.manual_seed(10)
    b = Discriminator(4, 64)
    for (k, v), w in zip(a.state_dict().items(), b.state_dict().values()):
        assert torch.equal(v, w), k
    torch.manual_seed(11)
    c = Discriminator(4, 64)
    assert not torch.equal(a._main[0].weight, c._main[0].weight)
    for i in (0, 2, 5, 8, 11):
        w = a._main[i].weight
        assert abs(float(w.std()) - 0.02) <= 0.1 * 0.02 and abs(float(w.mean())) <= 0.002, i
    for i in (3, 6, 9):
        assert abs(float(a._main[i].weight.mean()) - 1.0) <= 0.01 and bool((a._main[i].bias == 0).all())


def test_no_cpu_fallback_and_argument_rules():
    from spcl_amd import functional as F_hip
    from spcl_amd.semi_seg.arch.discr import Discriminator
    d = Discriminator(4, 8)
    x = torch.rand(1, 4, 64, 64)
    with pytest.raises(RuntimeError, match="MI355X"):
        d(x)
    with pytest.raises(RuntimeError, match="MI355X"):
        d.bce(x, 1)
    with pytest.raises(RuntimeError, match="MI355X"):
        F_hip.patch4s2_rows(x)
    with pytest.raises(RuntimeError, match="MI355X"):
        F_hip.rows_bn_stats(torch.rand(8, 4), torch.ones(4), torch.zeros(4), F_hip.RowsBN(None, None, True))
    with pytest.raises(ValueError, match="multiple of 4"):
        Discriminator(4, 6)
    assert int(d._main[3].num_batches_tracked) == 0  # a refused call counted nothing


def test_adversarial_trainer_builds_on_the_cpu():
    from spcl_amd.contrastyou.losses.kl import KL_div
    from spcl_amd.semi_seg.arch import UNet
    from spcl_amd.semi_seg.arch.discr import Discriminator
    from spcl_amd.semi_seg.epochers.adversarial import AdversarialEpocher
    from spcl_amd.semi_seg.trainers.semi import AdversarialTrainer, MixUpTrainer, SemiTrainer
    with pytest.raises(NotImplementedError):
        MixUpTrainer()
    with pytest.raises(NotImplementedError):  # the same refusal
        AdversarialTrainer()
    model = UNet(input_dim=1, num_classes=4, max_channel=128)
    kw = dict(model=model, labeled_loader=[], unlabeled_loader=[], val_loader=[], test_loader=None, criterion=KL_div(),
              save_dir=None, max_epoch=1, num_batches=1, device="cpu")
    with pytest.raises(TypeError, match="reg_weight"):
        AdversarialTrainer(**kw)
    before = torch.random.get_rng_state()
    tr = AdversarialTrainer(**kw, reg_weight=0.5, config={"RandomSeed": 7})
    assert torch.equal(torch.random.get_rng_state(), before)  # built under the configured seed, generators put back
    assert isinstance(tr, SemiTrainer) and tr.train_epocher is AdversarialEpocher and not tr.activate_hooks
    assert isinstance(tr._discriminator, Discriminator) and tr._discriminator._input_dim == 4 and tr._reg_weight == 0.5
    torch.manual_seed(7)
    want = Discriminator(4, 64)
    assert torch.equal(tr._discriminator._main[0].weight, want._main[0].weight)
    tr5 = AdversarialTrainer(**kw, reg_weight=0.0, dis_consider_image=True)
    assert tr5._discriminator._input_dim == 5 and tr5._discriminator._hidden_dim == 64
