"""GPU: the two mix-up kernels of csrc/semi_reg.hip.

``mixup_images`` must equal the CPU f32 expression ``lam * x + (1 - lam) * x[index]`` (``lam`` a ``np.float64``, as the
reference holds it) BIT FOR BIT: torch evaluates it as two products and one sum, each a correctly rounded IEEE f32 operation on
the f32 roundings of ``lam`` and ``1 - lam``, and the kernel performs the same three operations -- equality is the derived bar.
Sample sizes that take the 16-byte path, the 4-byte path (255 elements, or a view that starts one element into a buffer, on
either side), more than one workgroup per sample (224 x 224), a permutation that crosses the two halves and keeps a fixed
point.  The inputs are left as they were.

``mixup_kl_onehot``: loss within 1e-5 relative and gradient within 1e-5 relative L2 of float64 autograd of
``weight * kl_div(softmax(x64), mixed_y64)`` -- the bars tests/test_gpu_semi_reg_kernels.py holds the sibling criteria to --,
at 2880 pixels (12 workgroups, the last partial), fewer pixels than one workgroup, 16 classes and one full-size map; two runs
give the same bits; a label outside [0, C) selects no class."""
import types

import numpy as np
import pytest
import torch

from tests import _mixup_oracle as M

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
LAMS = [0.23538938957272115, 1.0, 3.7816489242002753e-4]


def _rel_l2(a, b):
    a, b = a.double().cpu(), b.double().cpu()
    return float((a - b).norm() / b.norm().clamp_min(1e-300))


def _perm(n2):
    """sample 0 stays, samples 1 and B trade places across the halves, the rest (if any) rotate; two samples just trade"""
    if n2 == 2:
        return torch.tensor([1, 0])
    b = n2 // 2
    p = list(range(n2))
    p[1], p[b] = p[b], p[1]
    rest = [k for k in range(n2) if k not in (0, 1, b)]
    for k, r in enumerate(rest):
        p[r] = rest[(k + 1) % len(rest)]
    assert sorted(p) == list(range(n2)) and p[0] == 0  # a permutation with a fixed point ...
    assert any((k < b) != (p[k] < b) for k in range(n2))  # ... that pairs samples across the two halves
    return torch.tensor(p)


def _offset_view(t, off):
    """``t`` on the device as a view that starts ``off`` elements into a larger buffer"""
    buf = torch.empty(off + t.numel() + 3, dtype=t.dtype, device=DEV)
    buf[off:off + t.numel()].copy_(t.reshape(-1))
    v = buf[off:off + t.numel()].view(t.shape)
    assert v.data_ptr() % 16 == (4 * off) % 16
    return v


IMAGE_CASES = [(shape, offs) for shape in [(3, 1, 20, 24), (3, 1, 15, 17), (2, 3, 8, 8)] for offs in [(0, 0), (1, 0), (0, 1)]]
IMAGE_CASES.append(((5, 1, 224, 224), (0, 0)))


@pytest.mark.parametrize("lam", LAMS)
@pytest.mark.parametrize("shape,offs", IMAGE_CASES)
def test_mixup_images_bit_identical_to_torch(shape, offs, lam):
    from spcl_amd import functional as F_hip
    g = torch.Generator().manual_seed(sum(shape) + 7 * offs[0] + 13 * offs[1])
    img, img_tf = torch.rand(*shape, generator=g), torch.rand(*shape, generator=g) - 0.5
    index = _perm(2 * shape[0])
    lam = np.float64(lam)
    x = torch.cat([img, img_tf], dim=0)
    want = lam * x + (1 - lam) * x[index, :]
    assert want.dtype == torch.float32
    # ... which is three f32 roundings on the f32 scalars, and is not the fused multiply-add's two
    l32, o32 = torch.tensor(lam, dtype=torch.float32), torch.tensor(1 - lam, dtype=torch.float32)
    assert torch.equal(want, l32 * x + o32 * x[index, :])
    a, b = _offset_view(img, offs[0]), _offset_view(img_tf, offs[1])
    plan = F_hip.MixupPlan(index, lam, DEV)
    got = F_hip.mixup_images(a, b, plan)
    assert got.shape == want.shape and got.dtype == torch.float32
    assert torch.equal(got.cpu(), want)
    assert torch.equal(a.cpu(), img) and torch.equal(b.cpu(), img_tf)  # the inputs are data: untouched


def test_mixup_images_refuses_what_it_cannot_index():
    from spcl_amd import functional as F_hip
    from spcl_amd import native as _n
    from ctypes import c_float
    img = torch.rand(2, 1, 8, 8, device=DEV)
    with pytest.raises(ValueError):
        F_hip.mixup_images(img, img.clone(), F_hip.MixupPlan([0, 1, 2, 3, 4, 5], 0.5, DEV))  # a plan for another batch size
    with pytest.raises(ValueError):
        F_hip.mixup_images(img, torch.rand(2, 1, 8, 4, device=DEV), F_hip.MixupPlan([0, 1, 2, 3], 0.5, DEV))
    plan = F_hip.MixupPlan([0, 1, 2, 3], 0.5, DEV)
    buf = torch.zeros(4 * 64, device=DEV)
    with pytest.raises(RuntimeError, match="overlaps"):  # refused on the host, nothing is launched
        _n.call("spcl_mixup_images", _n.ptr(buf[64:]), _n.ptr(img), _n.ptr(plan.index), 4, 64, c_float(0.5), c_float(0.5),
                _n.ptr(buf), _n.stream())


def _labels(shape, seed):
    """two label maps; the second view's agrees with the first's at about half of the pixels, so that whatever the
    permutation pairs, labels that agree and labels that differ both occur"""
    n2, c, h, w = shape
    g = torch.Generator().manual_seed(seed)
    tgt = torch.randint(0, c, (n2 // 2, 1, h, w), generator=g)
    other = torch.randint(0, c, (n2 // 2, 1, h, w), generator=g)
    keep = torch.rand(n2 // 2, 1, h, w, generator=g) < 0.5
    return tgt, torch.where(keep, tgt, other)


_REF = {}


def _reference(shape, lam, weight, tweak=None):
    """float64 loss and d(loss)/d(logits), computed once per case"""
    key = (shape, lam, weight, tweak)
    if key not in _REF:
        g = torch.Generator().manual_seed(sum(shape))
        x = torch.randn(*shape, generator=g)
        tgt, tgt_tf = _labels(shape, 3 + sum(shape))
        if tweak is not None:
            tgt, tgt_tf = tgt.clone(), tgt_tf.clone()
            tgt[0, 0, 0, :3] = tweak
            tgt_tf[-1, 0, -1, -2:] = tweak
        index = _perm(shape[0])
        x64 = x.double().requires_grad_(True)
        ref = weight * M.mixup_loss(x64, tgt, tgt_tf, lam, index)
        ref.backward()
        _REF[key] = (x, tgt, tgt_tf, index, float(ref.detach()), x64.grad)
    return _REF[key]


def _cl(x):
    return x.to(DEV).contiguous(memory_format=torch.channels_last)


@pytest.mark.parametrize("weight", [1.0, 2.5])
@pytest.mark.parametrize("lam", LAMS)
@pytest.mark.parametrize("shape", [(6, 4, 20, 24), (6, 2, 9, 13), (2, 16, 5, 7), (10, 4, 224, 224)])
def test_mixup_kl_onehot_vs_float64(shape, lam, weight):
    from spcl_amd import functional as F_hip
    x, tgt, tgt_tf, index, ref, gref = _reference(shape, lam, weight)
    la = torch.cat([tgt, tgt_tf]).squeeze(1)
    lb = la[index]
    assert bool((la == lb).any()) and bool((la != lb).any())  # both agreeing and disagreeing label pairs occur
    plan = F_hip.MixupPlan(index, lam, DEV)
    runs = []
    for _ in range(2):
        xd = _cl(x).requires_grad_(True)
        loss = F_hip.mixup_kl_onehot(xd, tgt.to(DEV), tgt_tf.to(DEV), plan, 1e-16, weight)
        loss.backward()
        runs.append((loss.detach().clone(), xd.grad.clone()))
    lerr = abs(float(runs[0][0]) - ref) / ref
    gerr = _rel_l2(runs[0][1], gref)
    print(f"mixup_kl_onehot {shape} lam={lam} weight={weight}: loss rel {lerr:.2e}, grad rel L2 {gerr:.2e}")
    assert lerr <= 1e-5 and gerr <= 1e-5, (lerr, gerr)
    assert torch.equal(runs[0][0], runs[1][0]) and torch.equal(runs[0][1], runs[1][1])


def test_mixup_kl_onehot_takes_squeezed_targets_and_scales_a_non_unit_gradient():
    from spcl_amd import functional as F_hip
    shape, lam = (6, 4, 20, 24), LAMS[0]
    x, tgt, tgt_tf, index, ref, gref = _reference(shape, lam, 1.0)
    plan = F_hip.MixupPlan(index, lam, DEV)
    xd = _cl(x).requires_grad_(True)
    loss = F_hip.mixup_kl_onehot(xd, tgt.squeeze(1).to(DEV), tgt_tf.squeeze(1).to(DEV), plan)
    (3.0 * loss).backward()
    assert abs(float(loss) - ref) <= 1e-5 * ref
    assert _rel_l2(xd.grad, 3.0 * gref) <= 1e-5
    # the backward itself: a registered unit gradient hands the launch's buffer on as it is, anything else scales a copy
    dl = torch.randn(6, 20, 24, 4, device=DEV)
    ctx = types.SimpleNamespace(saved_tensors=(dl,))
    unit = F_hip.register_unit_gradient(torch.ones((), device=DEV))
    out = F_hip._MixupKLFn.backward(ctx, unit)
    assert out[0].data_ptr() == dl.data_ptr() and out[0].shape == (6, 4, 20, 24) and all(o is None for o in out[1:])
    out = F_hip._MixupKLFn.backward(ctx, torch.full((), 3.0, device=DEV))
    assert out[0].data_ptr() != dl.data_ptr() and torch.equal(out[0], (dl * 3.0).permute(0, 3, 1, 2))
    out = F_hip._MixupKLFn.backward(ctx, torch.ones((), device=DEV))  # (1.0 that nobody registered: multiplied)
    assert out[0].data_ptr() != dl.data_ptr() and torch.equal(out[0], dl.permute(0, 3, 1, 2))


@pytest.mark.parametrize("bad", [4, -1])
def test_a_label_outside_the_classes_selects_no_class(bad):
    from spcl_amd import functional as F_hip
    shape, lam = (6, 4, 20, 24), LAMS[0]
    x, tgt, tgt_tf, index, ref, gref = _reference(shape, lam, 1.0, tweak=bad)
    assert int((torch.cat([tgt, tgt_tf]) == bad).sum()) == 5
    plan = F_hip.MixupPlan(index, lam, DEV)
    xd = _cl(x).requires_grad_(True)
    loss = F_hip.mixup_kl_onehot(xd, tgt.to(DEV), tgt_tf.to(DEV), plan)
    loss.backward()
    torch.cuda.synchronize()
    assert abs(float(loss) - ref) <= 1e-5 * ref
    assert _rel_l2(xd.grad, gref) <= 1e-5
    assert ref != _reference(shape, lam, 1.0)[4]  # (the zeroed rows do change the value)


def test_mixup_kl_onehot_argument_checks():
    from spcl_amd import functional as F_hip
    tgt = torch.zeros(2, 1, 5, 7, dtype=torch.long, device=DEV)
    plan = F_hip.MixupPlan([1, 0, 3, 2], 0.5, DEV)
    with pytest.raises(RuntimeError, match="C <= 16"):
        F_hip.mixup_kl_onehot(torch.zeros(4, 17, 5, 7, device=DEV), tgt, tgt, plan)
    with pytest.raises(RuntimeError, match="eps"):
        F_hip.mixup_kl_onehot(torch.zeros(4, 4, 5, 7, device=DEV), tgt, tgt, plan, eps=-1.0)
    with pytest.raises(ValueError):
        F_hip.mixup_kl_onehot(torch.zeros(4, 4, 5, 7, device=DEV), tgt, tgt[:1], plan)
    with pytest.raises(ValueError):
        F_hip.mixup_kl_onehot(torch.zeros(6, 4, 5, 7, device=DEV), tgt, tgt, plan)
