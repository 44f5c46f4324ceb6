"""GPU: the kernels of csrc/semi_reg.hip against float64 restatements.

``ema_update_``: k = 5 successive updates with the ramped ``alpha_t`` against the float64 formula, over sizes that reach the
16-byte body, the scalar tail and the scalar head (views that start one element into a buffer, on either side or both),
with and without the decay factor; the elements around the updated range stay untouched.  Bound (derived, not tuned): an
update rounds three times in f32, each by at most 2^-24 relative to a value no larger than max(|teacher|, |student|) -- the
result is a convex combination of the two, shrunk by the decay.  The kernel's f32 copies of alpha, 1 - alpha and 1 - decay
differ from the float64 values by |d_alpha| + |d_(1 - alpha)| + |d_(1 - decay)|, which the test computes for the values it
uses and checks to stay below 2^-24: at most 4 * 2^-24 * max per update, and an earlier update's error is carried on with
a factor alpha * (1 - decay) <= 1.

``mt_softmax_mse`` (teacher raw / soft-maxed, with and without flip flags) and ``entropy_softmax``: loss within 1e-5 relative
and gradient within 1e-5 relative L2 of float64 autograd -- the bars tests/test_gpu_iic_hooks.py holds the sibling
consistency kernel to -- at a small shape and at one full-size map; two runs give the same bits."""
import pytest
import torch
import torch.nn.functional as F

from tests import _iic_oracle as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
U = 2.0 ** -24


def _rel_l2(a, b):
    a, b = a.double().cpu(), b.double().cpu()
    return float((a - b).norm() / b.norm().clamp_min(1e-300))


def _alpha_t(step, alpha=0.999):
    return min(1 - 1 / (step + 1), alpha)


@pytest.mark.parametrize("decay", [1e-5, 0.0])
@pytest.mark.parametrize("t_off,s_off", [(0, 0), (1, 1), (1, 0), (0, 1)])
@pytest.mark.parametrize("n", [1, 7, 4096, 1310723])
def test_ema_update_vs_float64(n, t_off, s_off, decay):
    from spcl_amd import functional as F_hip
    k, guard = 5, 8
    g = torch.Generator().manual_seed(n + 10 * t_off + 100 * s_off)
    tbuf = torch.randn(t_off + n + guard, generator=g)
    students = [torch.randn(s_off + n, generator=g) for _ in range(k)]
    tdev = tbuf.to(DEV)
    tview = tdev[t_off:t_off + n]
    assert tview.data_ptr() % 16 == (4 * t_off) % 16
    ref = tbuf[t_off:t_off + n].double()
    mag = ref.abs()
    for step, s in enumerate(students):
        sdev = s.to(DEV)[s_off:]
        assert sdev.data_ptr() % 16 == (4 * s_off) % 16
        a = _alpha_t(step)
        assert sum(abs(float(torch.tensor(v, dtype=torch.float32)) - v) for v in (a, 1 - a, 1 - decay)) <= U
        F_hip.ema_update_(tview, sdev, a, decay)
        ref = (a * ref + (1 - a) * s[s_off:].double()) * (1 - decay)
        mag = torch.maximum(mag, s[s_off:].double().abs())
    got = tdev.cpu()
    err = (got[t_off:t_off + n].double() - ref).abs()
    bound = 4 * k * U * mag
    worst = float((err / bound.clamp_min(1e-300)).max())
    print(f"ema n={n} offsets=({t_off},{s_off}) decay={decay}: max err / bound = {worst:.3f}")
    assert bool((err <= bound).all()), worst
    assert torch.equal(got[:t_off], tbuf[:t_off]) and torch.equal(got[t_off + n:], tbuf[t_off + n:])


def test_ema_update_rejects_what_it_cannot_update_in_place():
    from spcl_amd import functional as F_hip
    t = torch.zeros(8, 8, device=DEV)
    with pytest.raises(ValueError):
        F_hip.ema_update_(t.t(), torch.zeros(8, 8, device=DEV), 0.5, 0.0)
    with pytest.raises(ValueError):
        F_hip.ema_update_(t, torch.zeros(8, 4, device=DEV), 0.5, 0.0)
    with pytest.raises(RuntimeError):
        F_hip.ema_update_(t, t, 0.5, 0.0)  # overlapping buffers
    with pytest.raises(RuntimeError):
        F_hip.ema_update_(torch.zeros(4), torch.zeros(4), 0.5, 0.0)  # no CPU path


def _mt64(t, s64, weight, flags, teacher_softmax):
    tt = R.flip(t.double(), flags)
    if teacher_softmax:
        tt = tt.softmax(1)
    return weight * F.mse_loss(tt.detach(), s64.softmax(1))


def _cl(x):
    return x.to(DEV).contiguous(memory_format=torch.channels_last)


@pytest.mark.parametrize("teacher_softmax", [False, True])
@pytest.mark.parametrize("shape,flags", [((3, 4, 20, 24), [3, 0, 1]), ((3, 4, 20, 24), None),
                                         ((10, 4, 224, 224), [3, 0, 1, 2, 0, 3, 1, 2, 0, 3])])
def test_mt_softmax_mse_vs_float64(shape, flags, teacher_softmax):
    from spcl_amd import functional as F_hip
    g = torch.Generator().manual_seed(7)
    t = torch.randn(*shape, generator=g)
    s = torch.randn(*shape, generator=g)
    weight = 1.0 if flags is None else 2.5
    fl = None if flags is None else torch.tensor(flags, dtype=torch.uint8, device=DEV)
    runs = []
    for _ in range(2):
        sd = _cl(s).requires_grad_(True)
        loss = F_hip.mt_softmax_mse(_cl(t), sd, weight, fl, teacher_softmax=teacher_softmax)
        loss.backward()
        runs.append((loss.detach().clone(), sd.grad.clone()))
    s64 = s.double().requires_grad_(True)
    ref = _mt64(t, s64, weight, flags, teacher_softmax)
    ref.backward()
    lerr = abs(float(runs[0][0]) - float(ref)) / float(ref)
    gerr = _rel_l2(runs[0][1], s64.grad)
    print(f"mt_softmax_mse {shape} flags={flags is not None} softmax={teacher_softmax}: loss rel {lerr:.2e}, grad rel L2 {gerr:.2e}")
    assert lerr <= 1e-5 and gerr <= 1e-5, (lerr, gerr)
    assert torch.equal(runs[0][0], runs[1][0]) and torch.equal(runs[0][1], runs[1][1])


def test_mt_softmax_mse_scales_a_non_unit_gradient_and_leaves_the_teacher_alone():
    from spcl_amd import functional as F_hip
    g = torch.Generator().manual_seed(8)
    t, s = torch.randn(2, 4, 9, 11, generator=g), torch.randn(2, 4, 9, 11, generator=g)
    td, sd = _cl(t).requires_grad_(True), _cl(s).requires_grad_(True)
    (3.0 * F_hip.mt_softmax_mse(td, sd)).backward()
    s64 = s.double().requires_grad_(True)
    (3.0 * _mt64(t, s64, 1.0, None, False)).backward()
    assert td.grad is None
    assert _rel_l2(sd.grad, s64.grad) <= 1e-5


@pytest.mark.parametrize("shape", [(3, 4, 20, 24), (10, 4, 224, 224)])
def test_entropy_softmax_vs_float64(shape):
    from spcl_amd import functional as F_hip
    from spcl_amd.contrastyou.losses.kl import Entropy
    g = torch.Generator().manual_seed(9)
    x = torch.randn(*shape, generator=g)
    weight = 0.7
    runs = []
    for _ in range(2):
        xd = _cl(x).requires_grad_(True)
        loss = F_hip.entropy_softmax(xd, 1e-16, weight)
        loss.backward()
        runs.append((loss.detach().clone(), xd.grad.clone()))
    x64 = x.double().requires_grad_(True)
    ref = weight * Entropy()(x64.softmax(1))
    ref.backward()
    lerr = abs(float(runs[0][0]) - float(ref)) / float(ref)
    gerr = _rel_l2(runs[0][1], x64.grad)
    print(f"entropy_softmax {shape}: loss rel {lerr:.2e}, grad rel L2 {gerr:.2e}")
    assert lerr <= 1e-5 and gerr <= 1e-5, (lerr, gerr)
    assert torch.equal(runs[0][0], runs[1][0]) and torch.equal(runs[0][1], runs[1][1])
    # the float path of the restated criterion on the device agrees as well
    dev = weight * Entropy()(_cl(x).softmax(1))
    assert abs(float(dev) - float(ref)) <= 1e-5 * float(ref)


@pytest.mark.parametrize("shape,flags", [((3, 4, 20, 24), [3, 0, 1]),   # 1440 pixels: six workgroups, the last partly empty
                                         ((3, 4, 20, 24), None),
                                         ((2, 2, 5, 7), [2, 1]),         # below one workgroup, C = 2
                                         ((1, 16, 9, 33), [3]),          # the maximum C
                                         # 288 workgroups: the closing sum fetches a second, partial batch of 32 partials
                                         ((2, 4, 192, 192), [1, 2])])
def test_consistency_is_the_soft_teacher_criterion_bit_for_bit(shape, flags):
    """``consistency_softmax_mse`` and ``mt_softmax_mse(teacher_softmax=True)`` are one launch of one kernel: the same bits"""
    from spcl_amd import functional as F_hip
    g = torch.Generator().manual_seed(12)
    a, b = torch.randn(*shape, generator=g), torch.randn(*shape, generator=g)
    fl = None if flags is None else torch.tensor(flags, dtype=torch.uint8, device=DEV)
    runs = []
    for criterion in (F_hip.consistency_softmax_mse, lambda *args: F_hip.mt_softmax_mse(*args, teacher_softmax=True)):
        bd = _cl(b).requires_grad_(True)
        loss = criterion(_cl(a), bd, 2.5, fl)
        (3.0 * loss).backward()
        runs.append((loss.detach().clone(), bd.grad.clone()))
    assert torch.equal(runs[0][0], runs[1][0]) and torch.equal(runs[0][1], runs[1][1])
