"""GPU: csrc/sup_dice.hip (``DiceKLLoss.from_logits`` / ``forward``) against the float64 autograd oracle of
tests/_sup_dice_oracle.py on the same float32 logits.

Bars, the ones tests/test_gpu_semi_reg_kernels.py holds the sibling per-pixel criteria to: loss within 1e-5 relative, gradient
within 1e-5 relative L2.  Shapes: a ragged tail on the 16-byte path (C = 4), more than 256 workgroup rows (5 x 4 x 120 x 112:
265 workgroups), C = 5 (the eight-class build), C = 16 (the sixteen-class build), C = 2, and a single pixel -- crossed with logit
scales 1 and 12, ``per_sample`` x ``include_background``, class weights drawn from [0.1, 2.1], and the last class absent from
the labels.  The single pixel runs at unit scale only: saturated, 1 - dice cancels there and even a float32 torch formulation
misses 1e-5."""
import pytest
import torch

from tests import _sup_dice_oracle as O

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SHAPES = [(3, 4, 19, 23), (2, 4, 64, 64), (5, 4, 120, 112), (2, 5, 17, 31), (2, 16, 9, 13), (3, 2, 33, 7), (1, 2, 1, 1)]
CASES = [(s, sc) for s in SHAPES for sc in (1.0, 12.0) if not (s == (1, 2, 1, 1) and sc != 1.0)]
_INPUTS, _REFS = {}, {}


def _rel_l2(a, b):
    a, b = a.double().cpu(), b.double().cpu()
    return float((a - b).norm() / b.norm().clamp_min(1e-300))


def _inputs(shape, scale):
    """seeded (logits, labels, class weights) of a case, made once; the last class never occurs in the labels"""
    key = (shape, scale)
    if key not in _INPUTS:
        N, C, H, W = shape
        g = torch.Generator().manual_seed(1000 * N + 100 * C + H + int(scale))
        logits = scale * torch.randn(N, C, H, W, generator=g)
        labels = torch.randint(0, C - 1, (N, H, W), generator=g)
        weights = tuple((0.1 + 2.0 * torch.rand(C, generator=g)).tolist())
        _INPUTS[key] = (logits, labels, weights)
    return _INPUTS[key]


def _reference(shape, scale, per_sample, include_background, **kw):
    key = (shape, scale, per_sample, include_background, tuple(sorted(kw.items())))
    if key not in _REFS:
        logits, labels, weights = _inputs(shape, scale)
        args = dict(dice_weight=0.7, kl_weight=1.3, class_weight=weights, per_sample=per_sample,
                    include_background=include_background)
        args.update(kw)
        _REFS[key] = O.dice_kl_with_grad(logits, labels, **args)
    return _REFS[key]


def _cl(x):
    return x.to(DEV).contiguous(memory_format=torch.channels_last)


def _run(crit, logits, labels, upstream=None):
    x = _cl(logits).requires_grad_(True)
    loss = crit.from_logits(x, labels.to(DEV))
    if upstream is None:
        loss.backward()
    else:
        loss.backward(gradient=upstream)
    return loss.detach(), x.grad


@pytest.mark.parametrize("include_background", [True, False])
@pytest.mark.parametrize("per_sample", [False, True])
@pytest.mark.parametrize("shape,scale", CASES)
def test_loss_and_gradient_vs_float64(shape, scale, per_sample, include_background):
    from spcl_amd import functional as F_hip
    from spcl_amd.contrastyou.losses import DiceKLLoss
    logits, labels, weights = _inputs(shape, scale)
    ref_loss, ref_grad, ref_kl, ref_dice = _reference(shape, scale, per_sample, include_background)
    crit = DiceKLLoss(dice_weight=0.7, kl_weight=1.3, class_weight=weights, per_sample=per_sample,
                      include_background=include_background)
    loss, grad = _run(crit, logits, labels)
    e_loss = abs(float(loss) - float(ref_loss)) / abs(float(ref_loss))
    e_grad = _rel_l2(grad, ref_grad)
    l_kl, l_dice = (float(v) for v in crit.last_parts.cpu())
    print(f"sup_dice {shape} scale={scale} per_sample={per_sample} bg={include_background}: loss {float(loss):.7f} "
          f"rel err {e_loss:.2e}, grad rel L2 {e_grad:.2e}, parts ({l_kl:.6f}, {l_dice:.6f})")
    assert e_loss <= 1e-5, e_loss
    assert e_grad <= 1e-5, e_grad
    assert abs(l_kl - float(ref_kl)) <= 1e-5 * abs(float(ref_kl)) and abs(l_dice - float(ref_dice)) <= 1e-5 * abs(float(ref_dice))
    # the parts sum to the loss under the weights (float32 roundings of three stored values)
    assert abs(0.7 * l_dice + 1.3 * l_kl - float(loss)) <= 4 * 2.0 ** -24 * (0.7 * abs(l_dice) + 1.3 * abs(l_kl))
    # the Dice counts are those of the separate kernels, exactly
    inter, union = crit.last_counts
    ri, ru = F_hip.dice_counts(F_hip.argmax_classes(_cl(logits)), labels.to(DEV), shape[1])
    assert inter.dtype == torch.int64 and tuple(inter.shape) == (shape[0], shape[1])
    assert torch.equal(inter, ri) and torch.equal(union, ru)
    oi, ou = O.dice_counts(logits.argmax(1), labels, shape[1])
    assert torch.equal(inter.cpu(), oi) and torch.equal(union.cpu(), ou)


@pytest.mark.parametrize("kind", ["dice", "weighted_kl"])
@pytest.mark.parametrize("shape", [(3, 4, 19, 23), (2, 5, 17, 31)])
def test_single_term_criteria_vs_float64(shape, kind):
    from spcl_amd.contrastyou.losses import SoftDiceLoss, WeightedKL
    logits, labels, weights = _inputs(shape, 1.0)
    if kind == "dice":
        crit, kw = SoftDiceLoss(include_background=False, per_sample=True), dict(dice_weight=1.0, kl_weight=0.0, class_weight=None)
    else:
        crit, kw = WeightedKL(class_weight=weights), dict(dice_weight=0.0, kl_weight=1.0)
    ref_loss, ref_grad, _, _ = _reference(shape, 1.0, kind == "dice", kind != "dice", **kw)
    loss, grad = _run(crit, logits, labels)
    assert abs(float(loss) - float(ref_loss)) <= 1e-5 * abs(float(ref_loss))
    assert _rel_l2(grad, ref_grad) <= 1e-5


def test_unit_weights_without_dice_is_the_fused_kl_div():
    """w == 1, dice_weight = 0: the value of ``functional.sup_loss_kl_onehot`` (float32 sums there, float64 here)"""
    from spcl_amd import functional as F_hip
    from spcl_amd.contrastyou.losses import WeightedKL
    logits, labels, _ = _inputs((2, 4, 64, 64), 1.0)
    loss = WeightedKL().from_logits(_cl(logits), labels.to(DEV))
    ref, (ri, ru) = F_hip.sup_loss_kl_onehot(_cl(logits), labels.to(DEV))
    assert abs(float(loss) - float(ref)) <= 1e-5 * abs(float(ref))
    assert abs(float(loss) - float(O.kl_div_onehot(logits, labels))) <= 1e-6 * abs(float(ref))


@pytest.mark.parametrize("shape", [(3, 4, 19, 23), (2, 5, 17, 31)])
def test_out_of_range_labels_are_all_zero_rows(shape):
    from spcl_amd.contrastyou.losses import DiceKLLoss
    logits, labels, weights = _inputs(shape, 1.0)
    labels = labels.clone()
    labels[0, 0, :5], labels[-1, -1, -3:], labels[0, 3, 3] = 255, -1, shape[1]
    crit = DiceKLLoss(class_weight=weights, per_sample=True)
    loss, grad = _run(crit, logits, labels)
    ref_loss, ref_grad, _, _ = O.dice_kl_with_grad(logits, labels, class_weight=weights, per_sample=True)
    assert abs(float(loss) - float(ref_loss)) <= 1e-5 * abs(float(ref_loss))
    assert _rel_l2(grad, ref_grad) <= 1e-5
    oi, ou = O.dice_counts(logits.argmax(1), labels, shape[1])
    assert torch.equal(crit.last_counts[0].cpu(), oi) and torch.equal(crit.last_counts[1].cpu(), ou)


@pytest.mark.parametrize("shape", [(5, 4, 120, 112), (2, 16, 9, 13)])
def test_two_calls_give_the_same_bits(shape):
    from spcl_amd.contrastyou.losses import DiceKLLoss
    logits, labels, weights = _inputs(shape, 12.0)
    runs = []
    for _ in range(2):
        crit = DiceKLLoss(class_weight=weights, per_sample=True, include_background=False)
        loss, grad = _run(crit, logits, labels)
        runs.append((loss.clone(), grad.clone(), crit.last_parts.clone()))
    assert all(torch.equal(a, b) for a, b in zip(*runs))


def test_forward_on_probabilities_is_from_logits():
    from spcl_amd import functional as F_hip
    from spcl_amd.contrastyou.losses import DiceKLLoss
    from spcl_amd.contrastyou.losses.kl import class2one_hot
    logits, labels, weights = _inputs((2, 4, 64, 64), 1.0)
    crit = DiceKLLoss(class_weight=weights)
    direct = float(crit.from_logits(_cl(logits), labels.to(DEV)))
    prob, onehot = F_hip.softmax_classes(_cl(logits)), class2one_hot(labels.to(DEV), 4)
    for kw in ({}, {"disable_assert": True}):
        assert abs(float(crit(prob, onehot, **kw)) - direct) <= 1e-6 * abs(direct)
    with pytest.raises(AssertionError, match="one-hot"):
        crit(prob, prob)


def test_upstream_gradient_scales_the_gradient():
    from spcl_amd import functional as F_hip
    from spcl_amd.contrastyou.losses import DiceKLLoss
    shape = (3, 4, 19, 23)
    logits, labels, weights = _inputs(shape, 1.0)
    _, ref_grad, _, _ = _reference(shape, 1.0, False, True)
    crit = DiceKLLoss(dice_weight=0.7, kl_weight=1.3, class_weight=weights)
    _, g1 = _run(crit, logits, labels)
    _, g3 = _run(crit, logits, labels, upstream=torch.tensor(-2.5, device=DEV))
    assert _rel_l2(g3, -2.5 * ref_grad) <= 1e-5
    assert float((g3 - (-2.5) * g1).abs().max()) <= 2.0 ** -23 * float((2.5 * g1).abs().max())
    unit = F_hip.register_unit_gradient(torch.ones((), device=DEV))  # (the epochers' registered unit: no scaling)
    _, gu = _run(crit, logits, labels, upstream=unit)
    assert torch.equal(gu, g1)


def test_no_grad_runs_the_first_pass_only_and_saves_nothing():
    from spcl_amd.contrastyou.losses import DiceKLLoss
    logits, labels, weights = _inputs((3, 4, 19, 23), 1.0)
    crit, x, y = DiceKLLoss(class_weight=weights), _cl(logits).requires_grad_(True), labels.to(DEV)
    packed = []

    def pack(t):
        packed.append(tuple(t.shape))
        return t
    with torch.autograd.graph.saved_tensors_hooks(pack, lambda t: t):
        with torch.no_grad():
            quiet = crit.from_logits(x, y)
        assert packed == [] and quiet.grad_fn is None and not quiet.requires_grad
        loud = crit.from_logits(x, y)
        assert packed and loud.requires_grad
    assert torch.equal(quiet, loud.detach())


def test_one_call_captured_in_a_graph_replays_on_new_data():
    from spcl_amd.contrastyou.losses import DiceKLLoss
    shape = (5, 4, 120, 112)
    la, ya, weights = _inputs(shape, 1.0)
    lb, yb, _ = _inputs(shape, 12.0)
    crit = DiceKLLoss(dice_weight=0.7, kl_weight=1.3, class_weight=weights, per_sample=True)
    eager = [(_run(crit, l, y), [c.clone() for c in crit.last_counts]) for l, y in ((la, ya), (lb, yb))]
    sx, sy = _cl(la).requires_grad_(True), ya.to(DEV)
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
        counts = crit.last_counts
    for (l, y), ((e_loss, e_grad), e_counts) in zip(((lb, yb), (la, ya)), (eager[1], eager[0])):
        with torch.no_grad():
            sx.copy_(_cl(l))
            sy.copy_(y)
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(loss, e_loss) and torch.equal(grad, e_grad)
        assert torch.equal(counts[0], e_counts[0]) and torch.equal(counts[1], e_counts[1])
