"""GPU: csrc/boundary.hip against tests/_boundary_oracle.py.

Distance maps: ``functional.signed_distance_maps`` equals the scipy oracle bit for bit (``torch.equal``, no tolerance).  The
widths 70, 130 and 65 cross the 64-lane chunks with a remainder, 13 and 9 are no multiples of the column batch of 8, H = 1 and
W = 1 leave one of the two passes nothing to do, 1024 is the limit of the uint16 planes.

Criterion: ``BoundaryLoss`` against the float64 autograd oracle on the same float32 logits.  Loss:
|loss - ref| <= 1e-5 (|L_region,ref| + alpha A), A = mean |p phi| (L_B is a signed sum that may cancel); gradient: 1e-5 relative
L2 -- the bars of tests/test_gpu_sup_dice_kernels.py.  (3, 4, 640, 560) has more pixels than the 2048 workgroups of the forward
and the 4096 of the backward take in one pass: their grid-stride loops run."""
import pytest
import torch

from tests import _boundary_oracle as O

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
C_MAP = 4  # classes of the label fields below
MAP_SHAPES = [(1, 1, 1), (1, 1, 70), (1, 13, 1), (2, 13, 70), (1, 9, 130), (2, 37, 65), (1, 64, 64), (1, 2, 1024),
              (1, 1024, 3)]  # (H = 1024: the columns kernel's segments are full 64-bit masks)
FIELDS = ["random0.02", "random0.5", "random0.98", "blobs", "absent", "full", "corners", "checkerboard", "out_of_range"]
CLASS_LISTS = [(0, 1, 2, 3), (1, 2, 3), (2,)]
ALPHA = 0.37
_FIELDS, _REFS = {}, {}


def _blobs(N, H, W, g):
    """discs of the three foreground classes on background"""
    ys, xs = torch.meshgrid(torch.arange(H), torch.arange(W), indexing="ij")
    lab = torch.zeros(N, H, W, dtype=torch.long)
    for n in range(N):
        for k in range(5):
            cy, cx = (torch.rand(2, generator=g) * torch.tensor([H, W])).tolist()
            r = 1.0 + float(torch.rand((), generator=g)) * 0.3 * max(H, W)
            lab[n][(ys - cy) ** 2 + (xs - cx) ** 2 <= r * r] = 1 + k % 3
    return lab


def _field(shape, kind):
    key = (shape, kind)
    if key not in _FIELDS:
        N, H, W = shape
        g = torch.Generator().manual_seed(H * 10000 + W * 10 + N + len(kind))
        if kind.startswith("random"):
            p = float(kind[len("random"):])
            lab = torch.randint(1, C_MAP, shape, generator=g) * (torch.rand(shape, generator=g) < p)
        elif kind == "blobs":
            lab = _blobs(N, H, W, g)
        elif kind == "absent":  # class 2 never occurs
            lab = torch.tensor([0, 1, 3])[torch.randint(0, 3, shape, generator=g)]
        elif kind == "full":  # class 2 fills sample 0 (every other class is absent there)
            lab = torch.randint(0, C_MAP, shape, generator=g)
            lab[0] = 2
        elif kind == "corners":  # one object pixel in each corner
            lab = torch.zeros(shape, dtype=torch.long)
            lab[:, 0, 0], lab[:, 0, -1], lab[:, -1, 0], lab[:, -1, -1] = 1, 2, 3, 2
        elif kind == "checkerboard":
            ys, xs = torch.meshgrid(torch.arange(H), torch.arange(W), indexing="ij")
            lab = (1 + (ys + xs) % 2).expand(N, H, W).clone()
        else:  # labels outside [0, C) belong to no class
            lab = torch.randint(0, C_MAP, shape, generator=g)
            u = torch.rand(shape, generator=g)
            lab[u < 0.1], lab[(u >= 0.1) & (u < 0.2)], lab[(u >= 0.2) & (u < 0.3)] = 255, -1, C_MAP
        _FIELDS[key] = lab.long()
    return _FIELDS[key]


@pytest.mark.parametrize("kind", FIELDS)
@pytest.mark.parametrize("shape", MAP_SHAPES)
def test_distance_maps_equal_the_oracle(shape, kind):
    from spcl_amd import functional as F_hip
    lab = _field(shape, kind)
    ref_all = O.signed_distance_ref(lab, CLASS_LISTS[0])  # (a class's map does not depend on the list it is asked in)
    dev = lab.to(DEV)
    for classes in CLASS_LISTS:
        phi = F_hip.signed_distance_maps(dev, classes)
        assert phi.dtype == torch.float32 and tuple(phi.shape) == (shape[0], len(classes)) + shape[1:]
        assert phi.permute(0, 2, 3, 1).is_contiguous()  # channels-last, beside the logits
        got, ref = phi.cpu(), ref_all[:, list(classes)]
        assert torch.equal(got, ref), (classes, int((got != ref).sum()), float((got - ref).abs().max()))
    if kind == "full":
        assert not F_hip.signed_distance_maps(dev[:1], (0, 1, 2, 3)).any()  # class 2 full, the others absent: all zero


def test_distance_maps_at_224():
    from spcl_amd import functional as F_hip
    g = torch.Generator().manual_seed(224)
    lab = _blobs(1, 224, 224, g)
    lab[0, 100:103, 50:60] = 255
    for classes in CLASS_LISTS:
        got, ref = F_hip.signed_distance_maps(lab.to(DEV), classes).cpu(), O.signed_distance_ref(lab, classes)
        assert torch.equal(got, ref), (classes, int((got != ref).sum()))
    assert float(ref.abs().max()) > 20  # (the blobs leave far pixels: the row search runs long)


def test_two_map_calls_give_the_same_bits():
    from spcl_amd import functional as F_hip
    lab = _field((2, 37, 65), "random0.5").to(DEV)
    a, b = F_hip.signed_distance_maps(lab, (1, 2, 3)).clone(), F_hip.signed_distance_maps(lab, (1, 2, 3))
    assert torch.equal(a, b)


# ---- the criterion
LOSS_SHAPES = [(1, 2, 13, 70), (3, 4, 37, 65), (3, 5, 9, 130), (1, 16, 17, 31), (3, 4, 64, 64)]
LOSS_CASES = [(s, bg, given) for s in LOSS_SHAPES for bg in (True, False) for given in (False, True)]
LOSS_CASES.append(((3, 4, 640, 560), False, False))
_INPUTS = {}


def _rel_l2(a, b):
    a, b = a.double().cpu(), b.double().cpu()
    return float((a - b).norm() / b.norm().clamp_min(1e-300))


def _cl(x):
    return x.to(DEV).contiguous(memory_format=torch.channels_last)


def _inputs(shape):
    """seeded (logits, labels) of a shape, made once: discs of the foreground classes, some labels outside [0, C)"""
    if shape not in _INPUTS:
        N, C, H, W = shape
        g = torch.Generator().manual_seed(1000 * N + 100 * C + H)
        logits = 3.0 * torch.randn(N, C, H, W, generator=g)
        labels = _blobs(N, H, W, g) % C
        labels[0, 0, :3] = 255
        _INPUTS[shape] = (logits, labels)
    return _INPUTS[shape]


def _given(C):
    return (C - 1, 0) if C > 2 else (1,)


def _criterion(C, include_background, given, alpha=ALPHA, **kw):
    from spcl_amd.contrastyou.losses import BoundaryLoss, DiceKLLoss
    region = DiceKLLoss(dice_weight=0.7, kl_weight=1.3, include_background=include_background, per_sample=True)
    return BoundaryLoss(region=region, alpha=alpha, classes=_given(C) if given else None, **kw)


def _run(crit, logits, labels, upstream=None):
    x = _cl(logits).requires_grad_(True)
    loss = crit.from_logits(x, labels.to(DEV))
    loss.backward(gradient=upstream)
    return loss.detach(), x.grad


@pytest.mark.parametrize("shape,include_background,given", LOSS_CASES)
def test_loss_and_gradient_vs_float64(shape, include_background, given):
    logits, labels = _inputs(shape)
    C = shape[1]
    crit = _criterion(C, include_background, given)
    key = (shape, include_background, given)
    if key not in _REFS:
        _REFS[key] = O.boundary_loss_with_grad(logits, labels, alpha=crit.alpha, classes=_given(C) if given else None,
                                               dice_weight=0.7, kl_weight=1.3, include_background=include_background,
                                               per_sample=True)
    ref_loss, ref_grad, ref_region, ref_lb, ref_a = _REFS[key]
    loss, grad = _run(crit, logits, labels)
    bar = 1e-5 * (abs(float(ref_region)) + crit.alpha * float(ref_a))
    e_loss, e_grad = abs(float(loss) - float(ref_loss)), _rel_l2(grad, ref_grad)
    l_kl, l_dice, l_b = (float(v) for v in crit.last_parts.cpu())
    print(f"boundary {shape} bg={include_background} given={given}: loss {float(loss):.7f} err {e_loss:.2e} (bar {bar:.2e}, "
          f"{e_loss / bar * 1e-5:.2e} of the magnitudes), grad rel L2 {e_grad:.2e}, L_B {l_b:.6f} (A {float(ref_a):.4f})")
    assert e_loss <= bar, (e_loss, bar)
    assert e_grad <= 1e-5, e_grad
    assert abs(l_b - float(ref_lb)) <= 1e-5 * float(ref_a)
    assert abs(0.7 * l_dice + 1.3 * l_kl - float(ref_region)) <= 1e-5 * abs(float(ref_region))
    assert crit.last_counts is crit.region.last_counts and tuple(crit.last_parts.shape) == (3,)


def test_functional_entries_and_upstream_gradient():
    from spcl_amd import functional as F_hip
    shape = (3, 4, 37, 65)
    logits, labels = _inputs(shape)
    classes = (1, 2, 3)
    phi = F_hip.signed_distance_maps(labels.to(DEV), classes)
    alpha = torch.full((), 0.25, device=DEV)
    ref_lb, ref_a = O.boundary_terms(logits, O.signed_distance_ref(labels, classes), classes)
    grads = []
    for up in (None, torch.tensor(-2.5, device=DEV)):
        x = _cl(logits).requires_grad_(True)
        loss, mean = F_hip.boundary_loss(x, phi, classes, alpha, with_mean=True)
        assert not mean.requires_grad and abs(float(mean) - float(ref_lb)) <= 1e-5 * float(ref_a)
        assert abs(float(loss) - 0.25 * float(ref_lb)) <= 1e-5 * 0.25 * float(ref_a)
        loss.backward(gradient=up)
        grads.append(x.grad)
    assert float((grads[1] - (-2.5) * grads[0]).abs().max()) <= 2.0 ** -22 * float((2.5 * grads[0]).abs().max())
    with torch.no_grad():  # no gradient asked: nothing is saved, the value is the same
        quiet = F_hip.boundary_loss(_cl(logits), phi, classes, alpha)
    assert quiet.grad_fn is None and torch.equal(quiet, loss.detach())
    with pytest.raises(ValueError, match="classes"):
        F_hip.boundary_loss(_cl(logits), phi, (1, 2, 4), alpha)


@pytest.mark.parametrize("shape", [(3, 4, 37, 65), (3, 5, 9, 130)])
def test_alpha_zero_is_the_region_criterion_bit_for_bit(shape):
    logits, labels = _inputs(shape)
    crit = _criterion(shape[1], False, False, alpha=0.0, alpha_step=0.0)
    loss, grad = _run(crit, logits, labels)
    r_loss, r_grad = _run(crit.region, logits, labels)
    assert torch.equal(loss, r_loss) and torch.equal(grad, r_grad)
    assert float(crit.last_parts[2]) != 0.0  # (L_B itself is still reported)


@pytest.mark.parametrize("shape", [(3, 4, 64, 64), (1, 16, 17, 31), (3, 4, 640, 560)])
def test_two_calls_give_the_same_bits(shape):
    logits, labels = _inputs(shape)
    runs = []
    for _ in range(2):
        crit = _criterion(shape[1], True, False)
        loss, grad = _run(crit, logits, labels)
        runs.append((loss.clone(), grad.clone(), crit.last_parts.clone()))
    assert all(torch.equal(a, b) for a, b in zip(*runs))


def test_captured_call_replays_with_the_alpha_of_a_later_epoch():
    shape = (3, 4, 64, 64)
    logits, labels = _inputs(shape)
    crit = _criterion(4, False, False, alpha=0.01, alpha_step=0.05)
    sx, sy = _cl(logits).requires_grad_(True), labels.to(DEV)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):  # (warm-up outside the capture)
        torch.autograd.grad(crit.from_logits(sx, sy), sx)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        loss = crit.from_logits(sx, sy)
        (grad,) = torch.autograd.grad(loss, sx)
        parts = crit.last_parts
    key = crit.graph_key()
    seen = []
    for epoch in (1, 7, 3):
        crit.set_epoch(epoch)  # (no recapture: the kernels read the device scalar)
        assert crit.graph_key() == key
        graph.replay()
        torch.cuda.synchronize()
        fresh = _criterion(4, False, False, alpha=0.01, alpha_step=0.05)
        fresh.set_epoch(epoch)
        e_loss, e_grad = _run(fresh, logits, labels)
        assert abs(fresh.alpha - (0.01 + 0.05 * (epoch - 1))) < 1e-12
        assert torch.equal(loss, e_loss) and torch.equal(grad, e_grad) and torch.equal(parts, fresh.last_parts)
        seen.append(float(loss))
    assert len(set(seen)) == 3


def test_absent_and_full_slices_contribute_exactly_zero():
    """class 2 is absent in sample 0 and fills sample 1: decided on the device, phi is zero there and so is L_B"""
    from spcl_amd import functional as F_hip
    from spcl_amd.contrastyou.losses import BoundaryLoss
    g = torch.Generator().manual_seed(5)
    logits = 3.0 * torch.randn(2, 4, 37, 65, generator=g)
    labels = torch.tensor([0, 1, 3])[torch.randint(0, 3, (2, 37, 65), generator=g)]
    labels[1] = 2
    assert not F_hip.signed_distance_maps(labels.to(DEV), (2,)).any()
    crit = BoundaryLoss(alpha=0.5, classes=(2,))
    loss, grad = _run(crit, logits, labels)
    r_loss, r_grad = _run(crit.region, logits, labels)
    assert float(crit.last_parts[2]) == 0.0
    assert torch.equal(loss, r_loss) and torch.equal(grad, r_grad)


def test_forward_on_probabilities_is_from_logits():
    from spcl_amd import functional as F_hip
    from spcl_amd.contrastyou.losses.kl import class2one_hot
    logits, labels = _inputs((3, 4, 64, 64))
    labels = labels.clamp(0, 3)
    crit = _criterion(4, True, False)
    direct = float(crit.from_logits(_cl(logits), labels.to(DEV)))
    prob, onehot = F_hip.softmax_classes(_cl(logits)), class2one_hot(labels.to(DEV), 4)
    for kw in ({}, {"disable_assert": True}):
        assert abs(float(crit(prob, onehot, **kw)) - direct) <= 1e-5 * abs(direct)
    with pytest.raises(AssertionError, match="one-hot"):
        crit(prob, prob)
