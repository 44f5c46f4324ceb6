"""GPU: the discriminator's kernels (csrc/discr.hip) one by one at tiny shapes against float64 ``F.unfold`` / ``F.conv2d`` /
``F.batch_norm`` / ``binary_cross_entropy`` (tests/_adv_oracle.py).

Tolerances.  A value that is ONE rounded operation away from its inputs (the patch rows: a copy, a LeakyReLU, one fused
multiply-add) is compared element by element: identity mode bit for bit, the others within 4 float32 ulps of the operands'
magnitude (|scale x| + |shift|: the fused multiply-add and torch's multiply-then-add differ by one rounding of the product).
Everything that goes through a product or a long sum is bounded by ``_adv_oracle.bound``: relative L2 error against float64
at most 4 x that of torch's float32 CPU evaluation of the same expression, at least 1e-6.  Each test prints what it
measured."""
import ctypes

import pytest
import torch
import torch.nn.functional as F

from tests import _adv_oracle as A

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
EPS32 = float(torch.finfo(torch.float32).eps)


def _g(seed):
    return torch.Generator().manual_seed(seed)


def _check(name, got, f32, ref64):
    err, tol = A.rel_l2(got, ref64), A.bound(f32, ref64)
    print(f"{name}: rel L2 {err:.3e} (float32 CPU {A.rel_l2(f32, ref64):.3e}, bound {tol:.3e})")
    assert err <= tol, (name, err, tol)


def _affine(C, seed):
    """scale around 1, shift FAR from 0: a padded tap that read act(shift) instead of 0 would be off by ~3"""
    g = _g(seed)
    return 0.5 + torch.rand(C, generator=g), 3.0 + torch.rand(C, generator=g)


# ------------------------------------------------------------------------------------------------ patch rows
@pytest.mark.parametrize("C", [4, 5, 8])
@pytest.mark.parametrize("H,W", [(8, 12), (7, 10), (4, 4)])
def test_patch_rows_forward_and_backward(C, H, W):
    from spcl_amd import functional as F_hip
    N = 2
    x = torch.randn(N, C, H, W, generator=_g(C * 100 + H))
    scale, shift = _affine(C, 7)
    drows = torch.randn(N * (H // 2) * (W // 2), 16 * C, generator=_g(5))
    for mode in (0, 1, 2):
        sc, sh = (scale, shift) if mode == 2 else (None, None)
        u64 = A.transform(x.double(), mode, None if sc is None else sc.double(), None if sh is None else sh.double())
        ref = A.patch_rows(u64)
        # the same map in NCHW memory, in channels-last memory, and (C > 1) as two maps stacked along the channels
        layouts = {"nchw": (x.to(DEV), None), "nhwc": (x.to(DEV).permute(0, 2, 3, 1).contiguous().permute(0, 3, 1, 2), None)}
        if mode == 0:
            layouts["stacked"] = (x[:, :1].to(DEV), x[:, 1:].to(DEV).permute(0, 2, 3, 1).contiguous().permute(0, 3, 1, 2))
        for name, (a, b) in layouts.items():
            got = F_hip.patch4s2_rows(a, mode, None if sc is None else sc.to(DEV), None if sh is None else sh.to(DEV), x2=b)
            again = F_hip.patch4s2_rows(a, mode, None if sc is None else sc.to(DEV), None if sh is None else sh.to(DEV), x2=b)
            assert torch.equal(got, again), (name, mode)
            got = got.cpu()
            assert got.shape == ref.shape
            if mode == 0:
                assert torch.equal(got, ref.float()), (name, mode)
                continue
            mag = x.abs() * (sc.view(1, -1, 1, 1) if mode == 2 else 1.0) + (sh.view(1, -1, 1, 1) if mode == 2 else 0.0)
            tol = 4 * EPS32 * A.patch_rows(mag.double())  # 0 at a padded tap: it must be exactly 0 there
            worst = float(((got.double() - ref).abs() - tol).max())
            print(f"patch rows C={C} {H}x{W} mode {mode} {name}: max |err| - tol = {worst:.3e}")
            assert worst <= 0, (name, mode, worst)
        # backward (gather) against autograd of the oracle; in BN mode w.r.t. the BatchNorm output scale x + shift
        if mode == 2:
            leaf = (x.double() * sc.double().view(1, -1, 1, 1) + sh.double().view(1, -1, 1, 1)).requires_grad_(True)
            rows = A.patch_rows(F.leaky_relu(leaf, A.SLOPE))
            leaf32 = (x * sc.view(1, -1, 1, 1) + sh.view(1, -1, 1, 1)).requires_grad_(True)
            rows32 = A.patch_rows(F.leaky_relu(leaf32, A.SLOPE))
        else:
            leaf = x.double().requires_grad_(True)
            rows = A.patch_rows(A.transform(leaf, mode))
            leaf32 = x.clone().requires_grad_(True)
            rows32 = A.patch_rows(A.transform(leaf32, mode))
        (rows * drows.double()).sum().backward()
        (rows32 * drows).sum().backward()
        xs = x.to(DEV).permute(0, 2, 3, 1).contiguous()
        for c_lo in ((0, 1) if mode == 0 else (0,)):
            dx = F_hip.patch4s2_rows_backward(drows.to(DEV), (N, C, H, W), mode, None if mode == 0 else xs,
                                              None if sc is None else sc.to(DEV), None if sh is None else sh.to(DEV), c_lo=c_lo)
            dx2 = F_hip.patch4s2_rows_backward(drows.to(DEV), (N, C, H, W), mode, None if mode == 0 else xs,
                                               None if sc is None else sc.to(DEV), None if sh is None else sh.to(DEV), c_lo=c_lo)
            assert torch.equal(dx, dx2)
            _check(f"patch rows backward C={C} {H}x{W} mode {mode} c_lo {c_lo}", dx.permute(0, 3, 1, 2),
                   leaf32.grad[:, c_lo:], leaf.grad[:, c_lo:])


# ------------------------------------------------------------------------------------------------ a whole layer
def _grads(out, weight_of, *leaves):
    return torch.autograd.grad((out * weight_of).sum(), leaves)


def test_layer_leaky_conv_8_to_16():
    """rows + rows product: LeakyReLU(0.2) -> Conv2d(8, 16, 4, 2, 1) at 2 x 8 x 12: output, dX, dW"""
    from spcl_amd import functional as F_hip
    g = _g(11)
    x, w = torch.randn(2, 8, 8, 12, generator=g), 0.1 * torch.randn(16, 8, 4, 4, generator=g)
    gy = torch.randn(2, 16, 4, 6, generator=g)
    res = {}
    for dt in (torch.float64, torch.float32):
        xl, wl = x.to(dt).requires_grad_(True), w.to(dt).requires_grad_(True)
        y = A.conv4s2(A.transform(xl, 1), wl)
        res[dt] = (y.detach(),) + _grads(y, gy.to(dt), xl, wl)
    xd = x.to(DEV).permute(0, 2, 3, 1).contiguous().permute(0, 3, 1, 2).requires_grad_(True)
    wd = w.to(DEV).requires_grad_(True)
    y = F_hip.discr_conv(xd, wd, leaky_in=True)
    dx, dw = _grads(y, gy.to(DEV), xd, wd)
    for name, got, i in (("y", y, 0), ("dX", dx, 1), ("dW", dw, 2)):
        _check(f"layer 8->16 {name}", got, res[torch.float32][i], res[torch.float64][i])
    # a pass that keeps no weight gradient: same dX, nothing for the weight
    y2 = F_hip.discr_conv(xd, wd, leaky_in=True, weight_grads=False)
    dx2, dw2 = torch.autograd.grad((y2 * gy.to(DEV)).sum(), (xd, wd), allow_unused=True)
    assert torch.equal(dx2, dx) and dw2 is None


def test_layer_bn_conv_16_to_32():
    """BatchNorm2d (training) -> LeakyReLU(0.2) -> Conv2d(16, 32, 4, 2, 1) at 3 x 6 x 6: output, dX (full BatchNorm backward),
    dgamma, dbeta, dW"""
    from spcl_amd import functional as F_hip
    g = _g(12)
    x, w = 2.0 + torch.randn(3, 16, 6, 6, generator=g), 0.1 * torch.randn(32, 16, 4, 4, generator=g)
    gamma, beta = 0.5 + torch.rand(16, generator=g), torch.randn(16, generator=g)
    gy = torch.randn(3, 32, 3, 3, generator=g)
    res = {}
    for dt in (torch.float64, torch.float32):
        ls = [t.to(dt).requires_grad_(True) for t in (x, gamma, beta, w)]
        y = A.conv4s2(F.leaky_relu(A.batch_norm(ls[0], ls[1], ls[2]), A.SLOPE), ls[3])
        res[dt] = (y.detach(),) + _grads(y, gy.to(dt), *ls)
    ld = [x.to(DEV).permute(0, 2, 3, 1).contiguous().permute(0, 3, 1, 2).requires_grad_(True)]
    ld += [t.to(DEV).requires_grad_(True) for t in (gamma, beta, w)]
    rm, rv = torch.zeros(16, device=DEV), torch.ones(16, device=DEV)
    y = F_hip.discr_bn_conv(ld[0], ld[1], ld[2], ld[3], F_hip.RowsBN(rm, rv, True))
    got = (y,) + _grads(y, gy.to(DEV), *ld)
    for name, gv, i in zip(("y", "dX", "dgamma", "dbeta", "dW"), got, range(5)):
        _check(f"layer 16->32 {name}", gv, res[torch.float32][i], res[torch.float64][i])


# ------------------------------------------------------------------------------------------------ BatchNorm over rows
@pytest.mark.parametrize("M", [30, 2 * 28 * 28])
@pytest.mark.parametrize("C", [16, 128])
def test_rows_bn(M, C):
    from spcl_amd import functional as F_hip
    g = _g(M + C)
    x = 1.5 + 2.0 * torch.randn(M, C, generator=g)
    gamma, beta = 0.5 + torch.rand(C, generator=g), torch.randn(C, generator=g)
    du = torch.randn(M, C, generator=g)
    res = {}
    for dt in (torch.float64, torch.float32):
        xl, gl, bl = (t.to(dt).requires_grad_(True) for t in (x, gamma, beta))
        rm, rv = torch.zeros(C, dtype=dt), torch.ones(C, dtype=dt)
        y = A.batch_norm(xl, gl, bl, rm, rv)
        grads = _grads(y, du.to(dt), xl, gl, bl)
        A.batch_norm(xl.detach(), gl.detach(), bl.detach(), rm, rv)  # the second call's running statistics
        mean, var = xl.detach().mean(0), xl.detach().var(0, unbiased=False)
        inv = 1.0 / torch.sqrt(var + 1e-5)
        res[dt] = dict(mean=mean, invstd=inv, scale=gl.detach() * inv, shift=bl.detach() - mean * gl.detach() * inv, rm=rm, rv=rv,
                       dx=grads[0], dgamma=grads[1], dbeta=grads[2])
    xd, gd, bd = x.to(DEV), gamma.to(DEV), beta.to(DEV)
    rm, rv = torch.zeros(C, device=DEV), torch.ones(C, device=DEV)
    bn = F_hip.RowsBN(rm, rv, True)
    stats = F_hip.rows_bn_stats(xd, gd, bd, bn)
    stats2 = F_hip.rows_bn_stats(xd, gd, bd, bn)
    assert torch.equal(stats, stats2)  # bitwise reproducible
    dx, dgamma, dbeta = F_hip.rows_bn_backward(du.to(DEV).clone(), xd, gd, stats, True)
    dx2, dgamma2, dbeta2 = F_hip.rows_bn_backward(du.to(DEV).clone(), xd, gd, stats, True)
    assert torch.equal(dx, dx2) and torch.equal(dgamma, dgamma2) and torch.equal(dbeta, dbeta2)
    got = dict(mean=stats[0], invstd=stats[1], scale=stats[2], shift=stats[3], rm=rm, rv=rv, dx=dx, dgamma=dgamma, dbeta=dbeta)
    for k, v in got.items():
        _check(f"rows BatchNorm M={M} C={C} {k}", v, res[torch.float32][k], res[torch.float64][k])
    # eval mode: the running statistics, untouched
    keep = (rm.clone(), rv.clone())
    ev = F_hip.rows_bn_stats(xd, gd, bd, F_hip.RowsBN(rm, rv, False))
    assert torch.equal(rm, keep[0]) and torch.equal(rv, keep[1])
    inv = 1.0 / torch.sqrt(rv.double().cpu() + 1e-5)
    assert A.rel_l2(ev[2], gamma.double() * inv) <= 1e-6 and A.rel_l2(ev[3], beta.double() - rm.double().cpu() * gamma.double() * inv) <= 1e-6


# ------------------------------------------------------------------------------------------------ head
def _head_case(H, W, t_abs, seed, C=8, N=2):
    """a pre-BN map, eval-mode BatchNorm (a fixed affine), head weights scaled so that max |t| = t_abs"""
    g = _g(seed)
    x = torch.randn(N, C, H, W, generator=g)
    gamma, beta = 0.5 + torch.rand(C, generator=g), 0.5 * torch.randn(C, generator=g)
    rm, rv = 0.1 * torch.randn(C, generator=g), 0.5 + torch.rand(C, generator=g)
    w = torch.randn(1, C, 4, 4, generator=g)
    t = A.head_logits(F.leaky_relu(A.batch_norm(x.double(), gamma.double(), beta.double(), rm.double(), rv.double(), False),
                                   A.SLOPE), w.double())
    return x, gamma, beta, rm, rv, w * (t_abs / float(t.abs().max()))


@pytest.mark.parametrize("H,W", [(4, 4), (5, 6)])
@pytest.mark.parametrize("y", [0, 1])
def test_head_bce(H, W, y):
    from spcl_amd import functional as F_hip
    x, gamma, beta, rm, rv, w = _head_case(H, W, 10.0, 100 + H + y)
    res = {}
    for dt in (torch.float64, torch.float32):
        xl, wl = x.to(dt).requires_grad_(True), w.to(dt).requires_grad_(True)
        u = F.leaky_relu(A.batch_norm(xl, gamma.to(dt), beta.to(dt), rm.to(dt), rv.to(dt), False), A.SLOPE)
        d = torch.sigmoid(A.head_logits(u, wl))
        loss = A.bce(d, y)
        res[dt] = (loss.detach(), d.detach()) + torch.autograd.grad(0.7 * loss, (xl, wl))
    assert float(res[torch.float64][1].min()) < 1e-3 or float(res[torch.float64][1].max()) > 1 - 1e-3  # |t| reaches ~10
    xd = x.to(DEV).permute(0, 2, 3, 1).contiguous().permute(0, 3, 1, 2).requires_grad_(True)
    wd = w.to(DEV).requires_grad_(True)
    gd, bd = gamma.to(DEV).requires_grad_(True), beta.to(DEV).requires_grad_(True)
    bn = F_hip.RowsBN(rm.to(DEV), rv.to(DEV), False)
    loss = F_hip.discr_bn_head(xd, gd, bd, wd, bn, label=y)
    dx, dw = torch.autograd.grad(0.7 * loss, (xd, wd))
    with torch.no_grad():
        d = F_hip.discr_bn_head(xd, gd, bd, wd, bn)
        loss_again = F_hip.discr_bn_head(xd, gd, bd, wd, bn, label=y)
    assert torch.equal(loss_again, loss.detach()) and d.shape == (2, 1, H - 3, W - 3)
    for name, got, i in (("loss", loss, 0), ("sigmoid", d, 1), ("dX", dx, 2), ("dW", dw, 3)):
        _check(f"head {H}x{W} y={y} {name}", got, res[torch.float32][i], res[torch.float64][i])
    # without a weight gradient: the same dX, nothing else
    loss2 = F_hip.discr_bn_head(xd, gd, bd, wd, bn, label=y, weight_grads=False)
    dx2, dw2, dg2 = torch.autograd.grad(0.7 * loss2, (xd, wd, gd), allow_unused=True)
    assert torch.equal(dx2, dx) and dw2 is None and dg2 is None


def test_head_sigmoid_output_and_its_backward():
    """``Discriminator.forward``'s path: sigmoid(t) as the output, differentiated by the caller (moderate logits: d (1 - d) in
    float32 is as ill-conditioned near saturation in torch's formulation as here, which is what the fused loss avoids)"""
    from spcl_amd import functional as F_hip
    x, gamma, beta, rm, rv, w = _head_case(5, 6, 2.0, 77)
    gd_out = torch.randn(2, 1, 2, 3, generator=_g(78))
    res = {}
    for dt in (torch.float64, torch.float32):
        xl, wl = x.to(dt).requires_grad_(True), w.to(dt).requires_grad_(True)
        u = F.leaky_relu(A.batch_norm(xl, gamma.to(dt), beta.to(dt), rm.to(dt), rv.to(dt), False), A.SLOPE)
        d = torch.sigmoid(A.head_logits(u, wl))
        res[dt] = (d.detach(),) + _grads(d, gd_out.to(dt), xl, wl)
    xd = x.to(DEV).permute(0, 2, 3, 1).contiguous().permute(0, 3, 1, 2).requires_grad_(True)
    wd = w.to(DEV).requires_grad_(True)
    d = F_hip.discr_bn_head(xd, gamma.to(DEV), beta.to(DEV), wd, F_hip.RowsBN(rm.to(DEV), rv.to(DEV), False))
    dx, dw = _grads(d, gd_out.to(DEV), xd, wd)
    for name, got, i in (("sigmoid", d, 0), ("dX", dx, 1), ("dW", dw, 2)):
        _check(f"head output path {name}", got, res[torch.float32][i], res[torch.float64][i])


@pytest.mark.parametrize("y", [0, 1])
def test_head_bce_is_the_softplus_value_at_saturation(y):
    """|t| = 40: float32 sigmoid(t) is exactly 0 or 1 and the log-then-clamp form would report 100 (and no gradient); the
    loss here is finite and equals mean softplus(+-t)"""
    from spcl_amd import functional as F_hip
    x, gamma, beta, rm, rv, w = _head_case(5, 6, 40.0, 55)
    u = F.leaky_relu(A.batch_norm(x.double(), gamma.double(), beta.double(), rm.double(), rv.double(), False), A.SLOPE)
    t = A.head_logits(u, w.double())
    want = A.softplus_bce(t, y)
    assert float(t.abs().max()) > 39.9
    xd = x.to(DEV).permute(0, 2, 3, 1).contiguous().permute(0, 3, 1, 2)
    loss = F_hip.discr_bn_head(xd, gamma.to(DEV), beta.to(DEV), w.to(DEV), F_hip.RowsBN(rm.to(DEV), rv.to(DEV), False), label=y)
    t32 = A.head_logits(u.float(), w)
    print(f"saturated head y={y}: loss {float(loss):.6f}, softplus {float(want):.6f}")
    assert torch.isfinite(loss).item()
    assert abs(float(loss) - float(want)) <= max(4 * abs(float(A.softplus_bce(t32, y)) - float(want)), 1e-6 * float(want))


# ------------------------------------------------------------------------------------------------ argument checks
def test_bad_arguments_are_refused_before_any_launch():
    from spcl_amd import native as n
    L = n.lib()

    def err():
        return L.spcl_last_error().decode()

    x = torch.full((2, 4, 4, 8), 7.0, device=DEV)
    out = torch.full((64,), -5.0, device=DEV)
    ws = torch.zeros(1 << 16, dtype=torch.uint8, device=DEV)
    vec = torch.ones(8, device=DEV)
    st = n.stream()
    P = n.ptr
    # a channel count that is no multiple of 4 (hidden_dim = 6 gives 12, 24, 48 -- and 6 output columns)
    assert L.spcl_rows_bn_workspace_bytes(32, 6) == 0
    rc = L.spcl_rows_bn_forward(P(x), 32, 6, P(vec), P(vec), ctypes.c_float(1e-5), ctypes.c_float(0.1), None, None, P(out), P(ws),
                                ws.numel(), st)
    assert rc == -1 and "multiple of 4" in err()
    rc = L.spcl_discr_head_forward(P(x), 2, 4, 4, 6, P(vec), P(vec), P(vec), 1, P(out), P(out), P(out), None, P(ws), ws.numel(), st)
    assert rc == -1 and "multiple of 4" in err()
    # a map smaller than the head's 4 x 4 window
    assert L.spcl_discr_head_workspace_bytes(2, 3, 4, 8) == 0
    rc = L.spcl_discr_head_forward(P(x), 2, 3, 4, 8, P(vec), P(vec), P(vec), 1, P(out), P(out), P(out), None, P(ws), ws.numel(), st)
    assert rc == -1 and "4 x 4" in err()
    rc = L.spcl_discr_head_backward(P(x), 2, 3, 4, 8, P(vec), P(vec), P(vec), P(out), None, P(out), None, P(ws), ws.numel(), st)
    assert rc == -1 and "4 x 4" in err()
    # null pointers
    rc = L.spcl_patch4s2_rows_forward(None, 8, 128, 1, 32, 8, None, 0, 0, 0, 0, 0, 2, 4, 4, 0, None, None, P(out), st)
    assert rc == -1 and "null" in err()
    rc = L.spcl_patch4s2_rows_forward(P(x), 8, 128, 1, 32, 8, None, 0, 0, 0, 0, 0, 2, 4, 4, 2, None, None, P(out), st)
    assert rc == -1 and "scale" in err()
    rc = L.spcl_patch4s2_rows_backward(P(x), None, 2, 4, 4, 8, 0, 1, None, None, P(out), st)
    assert rc == -1 and "stored map" in err()
    rc = L.spcl_rows_bn_backward(None, P(x), 32, 8, P(vec), P(vec), 1, P(out), P(out), P(out), P(ws), ws.numel(), st)
    assert rc == -1 and "null" in err()
    rc = L.spcl_discr_head_forward(P(x), 2, 4, 4, 8, P(vec), P(vec), None, 1, P(out), P(out), P(out), None, P(ws), ws.numel(), st)
    assert rc == -1 and "null" in err()
    # a workspace that is too small
    rc = L.spcl_rows_bn_forward(P(x), 32, 8, P(vec), P(vec), ctypes.c_float(1e-5), ctypes.c_float(0.1), None, None, P(out), P(ws), 8, st)
    assert rc == -1 and "workspace" in err()
    torch.cuda.synchronize()
    assert bool((out == -5.0).all()) and bool((x == 7.0).all())  # nothing was launched
    # and the Python layer names the rule
    from spcl_amd.semi_seg.arch.discr import Discriminator
    with pytest.raises(ValueError, match="multiple of 4"):
        Discriminator(4, 6)
