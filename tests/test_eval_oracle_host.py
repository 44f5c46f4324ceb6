"""CPU: what tests/test_gpu_eval_parity.py relies on, checked on the reference alone -- the helper (tests/_eval_oracle.py)
and the conditions under which its bars mean something: float32 stays close to float64 on these weights, few pixels sit
on an arg-max tie, the stage-wise oracle IS the oracle, and the closed form csrc/bn.hip states for the eval-mode BatchNorm
backward is what autograd computes."""
import pytest
import torch
import torch.nn.functional as F

from oracle import spcl_oracle as O
from tests import _eval_oracle as E

NETWORK_SHAPES = [(3, 48, 32, 128), (2, 64, 64, 256), (1, 112, 80, 128), (2, 16, 16, 128), (2, 224, 224, 256)]


def test_eval_state_has_real_statistics_and_float32_values():
    sd = E.eval_state(128, 3, hw=(32, 32))
    plain = O.init_unet_state(1, 4, 128, seed=3, dtype=torch.float64)
    assert sd.keys() == plain.keys()
    rv = torch.cat([v for k, v in sd.items() if k.endswith("running_var")])
    rm = torch.cat([v for k, v in sd.items() if k.endswith("running_mean")])
    gm = torch.cat([sd[k[:-len("running_var")] + "weight"] for k in sd if k.endswith("running_var")])
    assert float(rv.min()) == 0.0 and int((rv == 0).sum()) == 2 and int((rm == 50.0).sum()) == 2
    assert float(rv[rv > 0].min()) < 0.05 and float(rm.abs().median()) > 0.01  # nothing like zeros / ones
    assert 0.15 < float((gm < 0).double().mean()) < 0.3 and float(gm.abs().max()) <= 1.1 * 1.5
    for k, v in sd.items():
        if v.is_floating_point():
            assert v.dtype == torch.float64 and torch.equal(v.float().double(), v), k
        else:
            assert int(v) == 1, k  # the calibration pass counted once
    again = E.eval_state(128, 3, hw=(32, 32))
    assert all(torch.equal(sd[k], again[k]) for k in sd)


@pytest.mark.parametrize("shape", NETWORK_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_float32_oracle_is_close_and_few_pixels_are_tied(shape):
    c = E.case(*shape)
    worst = max(c["f32_err"].values())
    logits = c["f64"]["Deconv_1x1"]
    low = E.low_margin(logits)
    share = float(low.double().mean())
    flips = int((c["f32"]["Deconv_1x1"].argmax(1) != logits.argmax(1))[~low].sum())
    print(f"\n[eval oracle] {shape}: float32 vs float64 worst stage {worst:.2e}, low-margin share {100 * share:.3f} %")
    assert worst <= 5e-5, c["f32_err"]
    assert share <= E.MARGIN_SHARE
    assert flips == 0


@pytest.mark.parametrize("shape", list(E.GRAD_VARIANT), ids=lambda s: "x".join(map(str, s)))
def test_gradient_cases_are_complete_and_leave_the_shared_case_alone(shape):
    """the eval-mode gradient cases of the GPU test.  (Whether float32 arithmetic takes every ReLU gate of a case the way
    float64 does -- ``E.grad_variant_is_clean`` -- depends on the machine's float32 convolutions, so it is reported here, not
    asserted: the GPU test caps every bar, whatever the float32 oracle says.)"""
    variant = E.GRAD_VARIANT[shape][0]
    gc = E.grad_case(*shape)
    worst = max(gc["f32_err"].items(), key=lambda kv: kv[1])
    print(f"\n[eval oracle] {shape} variant {variant}: float32 gradients, worst tensor {worst[0]} {worst[1]:.2e}")
    assert gc["variant"] == variant
    assert set(gc["grads"]) == {k for k, v in gc["case"]["sd"].items() if v.is_floating_point() and "running" not in k}
    assert all(bool(torch.isfinite(g).all()) and float(g.abs().max()) > 0 for g in gc["grads"].values())
    assert not gc["case"]["x"].requires_grad and not any(v.requires_grad for v in gc["case"]["sd"].values())


def test_plain_float32_batchnorm_is_the_oracle_forward():
    c = E.case(3, 48, 32, 128)
    with torch.no_grad():
        assert E.relmax(E._forward_plain(c["x"], c["sd"]), c["f64"]["Deconv_1x1"]) < 1e-12


@pytest.mark.parametrize("q", [None, O.BF16Emulation], ids=["f64", "bf16-emulation"])
def test_chained_stages_are_the_oracle_forward(q):
    sd = E.eval_state(128, 5, hw=(32, 48))
    x = torch.rand(2, 1, 32, 48, generator=torch.Generator().manual_seed(6)).double()
    outs = E.chain(x, sd, q=q)
    assert tuple(outs) == E.STAGES
    with torch.no_grad():
        for s in E.STAGES:
            ref = O.unet_forward(x, {k: v.clone() for k, v in sd.items()}, E.until_of(s), train=False, q=q)
            assert torch.equal(outs[s], ref), s
    # eval mode reads the statistics and leaves them alone
    sd2 = {k: v.clone() for k, v in sd.items()}
    E.chain(x, sd2, q=q)
    assert all(torch.equal(sd[k], sd2[k]) for k in sd)


@pytest.mark.parametrize("pool", [False, True])
def test_eval_batchnorm_backward_closed_form(pool):
    """csrc/bn.hip: `eval: dy = scale*dz`, A = B = 0 -- with dz the gradient behind the ReLU gate (and, pooled, routed to the
    window's first maximum); dgamma = sum dz (y - running_mean) invstd, dbeta = sum dz."""
    g = torch.Generator().manual_seed(9)
    N, C, H, W = 3, 12, 9, 10
    y = torch.randn(N, C, H, W, generator=g, dtype=torch.float64, requires_grad=True)
    gamma = (0.5 + torch.rand(C, generator=g, dtype=torch.float64))
    gamma[::5] *= -1
    gamma.requires_grad_(True)
    beta = (0.3 * torch.randn(C, generator=g, dtype=torch.float64)).requires_grad_(True)
    rm = torch.randn(C, generator=g, dtype=torch.float64)
    rv = torch.rand(C, generator=g, dtype=torch.float64) * 2
    rv[1] = 0.0
    eps = 1e-5
    z = F.batch_norm(y, rm, rv, gamma, beta, False, 0.1, eps)
    a = F.relu(z)
    out = F.max_pool2d(a, 2, 2) if pool else a
    dout = torch.randn(out.shape, generator=g, dtype=torch.float64)
    da, = torch.autograd.grad(out, a, dout, retain_graph=True)  # the pooling's routing alone
    out.backward(dout)
    invstd = 1.0 / (rv + eps).sqrt()
    scale = (gamma.detach() * invstd).view(1, C, 1, 1)
    dz = da * (z.detach() > 0)
    torch.testing.assert_close(y.grad, scale * dz, rtol=1e-12, atol=1e-14)
    yhat = (y.detach() - rm.view(1, C, 1, 1)) * invstd.view(1, C, 1, 1)
    torch.testing.assert_close(gamma.grad, (dz * yhat).sum((0, 2, 3)), rtol=1e-12, atol=1e-12)
    torch.testing.assert_close(beta.grad, dz.sum((0, 2, 3)), rtol=1e-12, atol=1e-12)
