"""CPU-only: the host side of the fused Adam / AdamW / SGD steps (optim.py, trainers' ``build_optimizer``): the four floats a
staged step uploads are torch's formulas, a CPU flat parameter keeps the ``torch.optim`` classes, the constructors refuse what
torch's refuse."""
import math

import numpy as np
import pytest
import torch

import spcl_amd  # noqa: F401
from spcl_amd import native
from spcl_amd import optim as O
from spcl_amd.semi_seg.trainers.pretrain import build_optimizer

STEPS = (1, 2, 5, 6, 1000)


def test_abi_version_carries_the_new_entry_points():
    assert native.ABI_VERSION >= 17
    for name in ("spcl_adam_step_scaled", "spcl_adam_apply_staged", "spcl_sgd_step_scaled", "spcl_sgd_apply_staged"):
        assert name in native._SIGNATURES


@pytest.mark.parametrize("decoupled", [False, True])
def test_adam_host_coefficients_are_torch_s_formulas(decoupled):
    """torch/optim/adam.py _single_tensor_adam: step_size = lr / (1 - beta1 ** step), bias_correction2_sqrt =
    (1 - beta2 ** step) ** 0.5, and the decoupled decay's factor 1 - lr * weight_decay, in double; the learning rate is taken
    as the float32 the device holds.  beta ** t by repeated squaring differs from ``**`` by at most ~t / 2 ulp."""
    b1, b2, lr, wd = 0.9, 0.999, 2e-3, 1e-2
    lrf = float(np.float32(lr))
    for t in STEPS:
        c = O.adam_coefficients(t, lr, b1, b2, wd, decoupled)
        assert len(c) == 4 and c[3] == float(t)
        np.testing.assert_allclose(c[0], lrf / (1 - b1 ** t), rtol=1e-12)
        np.testing.assert_allclose(c[1], (1 - b2 ** t) ** 0.5, rtol=1e-10)
        np.testing.assert_allclose(c[2], 1 - lrf * wd, rtol=1e-15)
        # the float32 the kernel reads is torch's double rounded once (lr's own rounding aside)
        np.testing.assert_allclose(np.float32(c[0]), lr / (1 - b1 ** t), rtol=1.01 * 2 ** -23)
    assert O.adam_coefficients(3, lr, b1, b2)[2] == 1.0  # no decay: the factor is exactly one


def test_sgd_host_coefficients():
    """SGD has no bias correction: the learning rate (as the device's float32) and the step count"""
    for t in STEPS:
        c = O.sgd_coefficients(t, 1e-3)
        assert c == [float(np.float32(1e-3)), 0.0, 0.0, float(t)]


@pytest.mark.parametrize("name", ["Adam", "AdamW", "SGD", "Adagrad", "RMSprop"])
def test_build_optimizer_on_a_cpu_parameter_keeps_torch_optim(name):
    p = torch.nn.Parameter(torch.zeros(8))
    opt = build_optimizer(name, p, {"lr": 1e-3, "weight_decay": 1e-5})
    assert type(opt) is getattr(torch.optim, name) and not O.is_fused(opt)


def test_build_optimizer_amsgrad_selects_torch_adam():
    p = torch.nn.Parameter(torch.zeros(8))
    opt = build_optimizer("Adam", p, {"lr": 1e-3, "amsgrad": True})
    assert type(opt) is torch.optim.Adam and opt.defaults["amsgrad"] is True
    with pytest.raises(KeyError):
        build_optimizer("NoSuchOptimizer", p, {"lr": 1e-3})


def test_fused_classes_share_one_name():
    for cls in (O.FusedRAdam, O.FusedAdam, O.FusedAdamW, O.FusedSGD):
        assert issubclass(cls, O.FusedOptimizer) and issubclass(cls, torch.optim.Optimizer)
    assert issubclass(O.FusedAdamW, O.FusedAdam)
    assert not O.is_fused(torch.optim.SGD([torch.nn.Parameter(torch.zeros(2))], lr=0.0))


def test_constructor_refusals():
    p = torch.nn.Parameter(torch.zeros(8))
    for cls in (O.FusedAdam, O.FusedAdamW):
        for bad in ({"lr": -1.0}, {"eps": -1e-8}, {"weight_decay": -1.0}, {"betas": (1.0, 0.999)}, {"betas": (0.9, -0.1)}):
            with pytest.raises(ValueError):
                cls([p], **bad)
    for bad in ({"lr": -1.0}, {"momentum": -0.1}, {"weight_decay": -1.0}, {"nesterov": True},
                {"nesterov": True, "momentum": 0.9, "dampening": 0.1}):
        with pytest.raises(ValueError):
            O.FusedSGD([p], **bad)
    # no CPU path: the refusal FusedRAdam gives
    for cls in (O.FusedRAdam, O.FusedAdam, O.FusedAdamW, O.FusedSGD):
        with pytest.raises(RuntimeError, match="MI355X"):
            cls([p])
    # contiguous fp32 only
    half = torch.nn.Parameter(torch.zeros(8, dtype=torch.float64))
    strided = torch.nn.Parameter(torch.zeros(4, 4).t()[1:])
    assert not strided.is_contiguous()
    for cls in (O.FusedAdam, O.FusedAdamW, O.FusedSGD):
        for q in (half, strided):
            with pytest.raises(TypeError):
                cls([q])


def test_defaults_are_torch_s():
    import inspect
    pairs = ((O.FusedAdam, torch.optim.Adam), (O.FusedAdamW, torch.optim.AdamW), (O.FusedSGD, torch.optim.SGD))
    for mine, ref in pairs:
        a, b = inspect.signature(mine.__init__).parameters, inspect.signature(ref.__init__).parameters
        for k, v in a.items():
            if k in ("self", "params"):
                continue
            assert k in b and v.default == b[k].default, (mine.__name__, k)
    assert math.isclose(inspect.signature(O.FusedAdamW.__init__).parameters["weight_decay"].default, 1e-2)
