"""GPU: the ``Discriminator`` module (five HIP layers) against the float64 ``nn.Sequential`` of tests/_adv_oracle.py carrying
the same weights: output, input gradient, every parameter gradient, running statistics and ``num_batches_tracked`` after one
and two forwards, ``eval()``.  64 x 64 is the smallest input the head accepts (64 -> 32 -> 16 -> 8 -> 4 -> 1).  Tolerance:
``_adv_oracle.bound`` (4 x the float32 CPU evaluation's own error, at least 1e-6); the measured values are printed."""
import pytest
import torch

from tests import _adv_oracle as A

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _check(name, got, f32, ref64):
    err, tol = A.rel_l2(got, ref64), A.bound(f32, ref64)
    print(f"{name}: rel L2 {err:.3e} (float32 CPU {A.rel_l2(f32, ref64):.3e}, bound {tol:.3e})")
    assert err <= tol, (name, err, tol)


def _build(input_dim, hidden=8, seed=5):
    from spcl_amd.semi_seg.arch.discr import Discriminator
    torch.manual_seed(seed)
    d = Discriminator(input_dim, hidden)
    with torch.no_grad():  # weights large enough for the output to leave 0.5, BatchNorm affines off their defaults
        for i in (0, 2, 5, 8, 11):
            d._main[i].weight.mul_(8.0)
        for i in (3, 6, 9):
            d._main[i].bias.normal_(0.0, 0.3)
    refs = {dt: A.load_into(A.discriminator(input_dim, hidden, dt), d.state_dict()).train() for dt in (torch.float64, torch.float32)}
    return d.to(DEV).train(), refs


def _run_reference(net, x, gout):
    xl = x.to(net[0].weight.dtype).requires_grad_(True)
    out = net(xl)
    grads = torch.autograd.grad((out * gout.to(out.dtype)).sum(), [xl] + list(net.parameters()))
    return out.detach(), grads[0], dict(zip([k for k, _ in net.named_parameters()], grads[1:]))


@pytest.mark.parametrize("input_dim,shape", [(4, (3, 64, 64)), (5, (3, 64, 64)), (4, (2, 64, 96))])
def test_discriminator_vs_float64_sequential(input_dim, shape):
    N, H, W = shape
    d, refs = _build(input_dim)
    g = torch.Generator().manual_seed(9)
    x = torch.rand(N, input_dim, H, W, generator=g)
    gout = torch.randn(N, 1, H // 16 - 3, W // 16 - 3, generator=g)
    want = {dt: _run_reference(net, x, gout) for dt, net in refs.items()}
    xd = x.to(DEV).requires_grad_(True)
    out = d(xd)
    assert out.shape == gout.shape
    params = dict(d.named_parameters())
    grads = torch.autograd.grad((out * gout.to(DEV)).sum(), [xd] + list(params.values()))
    _check("output", out, want[torch.float32][0], want[torch.float64][0])
    _check("input gradient", grads[0], want[torch.float32][1], want[torch.float64][1])
    for (k, _), gk in zip(params.items(), grads[1:]):
        kk = k.split(".", 1)[1]
        _check(f"gradient of {k}", gk, want[torch.float32][2][kk], want[torch.float64][2][kk])

    def stats_match(tag):
        s64, s32 = refs[torch.float64].state_dict(), refs[torch.float32].state_dict()
        for k, v in d.state_dict().items():
            kk = k.split(".", 1)[1]
            if k.endswith("num_batches_tracked"):
                assert int(v) == int(s64[kk]), (tag, k, int(v))
            elif "running" in k:
                _check(f"{tag} {k}", v, s32[kk], s64[kk])

    stats_match("after one forward")
    with torch.no_grad():
        out2 = d(xd * 0.5)
        for net in refs.values():
            net(x.to(net[0].weight.dtype) * 0.5)
    stats_match("after two forwards")
    assert int(d._main[3].num_batches_tracked) == 2
    # eval(): the running statistics, which stay as they are
    d.eval()
    before = {k: v.clone() for k, v in d.state_dict().items()}
    with torch.no_grad():
        oe = d(xd)
        oe2 = d(xd)
        we = {dt: net.eval()(x.to(dt)) for dt, net in refs.items()}
    assert torch.equal(oe, oe2) and not torch.equal(oe, out.detach())
    for k, v in d.state_dict().items():
        assert torch.equal(v, before[k]), k
    _check("eval output", oe, we[torch.float32], we[torch.float64])
    assert out2.shape == out.shape


def test_bce_is_the_loss_of_the_output_and_image_stacking_reads_in_place():
    """``bce(x, y)`` = BCELoss(forward(x), y) and ``image=`` = the concatenation, gradients included (w.r.t. the class map)"""
    d, refs = _build(5)
    g = torch.Generator().manual_seed(19)
    img, prob = torch.rand(3, 1, 64, 64, generator=g), torch.rand(3, 4, 64, 64, generator=g).softmax(1)
    want = {}
    for dt, net in refs.items():
        p = prob.to(dt).requires_grad_(True)
        loss = A.bce(net(torch.cat([img.to(dt), p], 1)), 0)
        want[dt] = (loss.detach(), torch.autograd.grad(loss, p)[0])
    pd = prob.to(DEV).permute(0, 2, 3, 1).contiguous().permute(0, 3, 1, 2).requires_grad_(True)  # channels-last, as softmax_classes returns
    loss = d.bce(pd, 0, image=img.to(DEV))
    gp = torch.autograd.grad(loss, pd)[0]
    _check("bce with image", loss, want[torch.float32][0], want[torch.float64][0])
    _check("bce with image, class-map gradient", gp, want[torch.float32][1], want[torch.float64][1])
    assert int(d._main[9].num_batches_tracked) == 1


def test_a_float32_sequential_checkpoint_loads_strictly():
    from spcl_amd.semi_seg.arch.discr import Discriminator
    ref = A.discriminator(4, 8, torch.float32)
    d = Discriminator(4, 8)
    d.load_state_dict({"_main." + k: v for k, v in ref.state_dict().items()}, strict=True)
    d.to(DEV).eval()
    x = torch.rand(2, 4, 64, 64)
    with torch.no_grad():
        got = d(x.to(DEV))
        want64 = A.load_into(A.discriminator(4, 8), d.state_dict()).eval()(x.double())
        want32 = ref.eval()(x)
    _check("loaded checkpoint, eval output", got, want32, want64)
