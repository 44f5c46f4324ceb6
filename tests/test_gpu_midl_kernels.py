"""GPU: the patch-wise IIC segmentation criterion (csrc/iic_patch.hip, functional.iic_patch_loss) against the float64
restatement of ``IIDSegmentationSmallPathLoss`` (tests/_midl_oracle.py), scale = 0.1.

Bars.  Per-patch losses: 1e-5 relative (1e-9 absolute for the few below 1e-4 in magnitude: the min-shift makes the losses
small).  Total loss: 1e-5 relative.  Gradients: relative L2 within ``max(1e-5, e32)`` where ``e32`` is the error of the SAME
oracle evaluated entirely in float32 on the CPU against its float64 evaluation -- the reference's own arithmetic: the kernels
add the joint exactly and run the criterion in float64, so they must be no worse.  1e-5 is the bar of
tests/test_gpu_iic_kernels.py; each test prints ``e32`` next to the kernel's error.  The float64 / float32 references of a
case are computed once and shared by the tests of that case."""
import functools

import pytest
import torch

from tests import _iic_oracle as R
from tests import _midl_oracle as M

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SCALE = 0.1

CASES = [  # (N, C, H, W, pad, patch, flags)
    (2, 4, 20, 24, 1, 8, [1, 2]),          # 20 regular patches
    (3, 4, 21, 27, 1, 8, [3, 0, 1]),       # 30 patches; irregular last start on both axes; a pixel in 3 x 3 patches
    (2, 2, 9, 7, 1, 16, [2, 1]),           # patch larger than the map: one clipped patch; C = 2
    (2, 4, 16, 16, 0, 16, None),           # exactly one patch; pad = 0; no flags
    (1, 5, 19, 33, 2, 10, [3]),            # C not a multiple of 4; pad = 2
    (2, 16, 12, 12, 1, 6, [0, 3]),         # the maximum C
    (2, 4, 21, 27, 1, 7, [1, 0]),          # odd patch: step 3; 48 patches
    (2, 4, 40, 56, 3, 16, [1, 0]),         # pad = 3; 24 patches
    (2, 4, 224, 224, 1, 32, [3, 0]),       # the workload's map: 169 patches
    (2, 4, 224, 224, 1, 1024, [1, 2]),     # the default configuration: one patch split over workgroups
    (1, 4, 6, 300, 1, 1024, [2]),          # wider than 256: two column passes in the joint, two column chunks in backward
]
IDS = [f"case{k + 1}" for k in range(len(CASES))]


def _rel_l2(a, b):
    a, b = a.double().cpu(), b.double().cpu()
    return float((a - b).norm() / b.norm().clamp_min(1e-300))


def _logits(N, C, H, W):
    g = torch.Generator().manual_seed(1)
    lx = torch.randn(N, C, H, W, generator=g)
    ly = torch.randn(N, C, H, W, generator=g)
    return lx.float(), ly.float()


@functools.lru_cache(maxsize=None)
def _reference(case):
    """float64 oracle of a case and the float32 oracle's gradient errors against it: (loss, per-patch, gx, gy, e32x, e32y)"""
    N, C, H, W, pad, patch, flags = CASES[case]
    lx, ly = _logits(N, C, H, W)
    loss, per_patch, gx, gy = M.evaluate(lx, ly, pad, patch, flags, SCALE, torch.float64)
    _, _, gx32, gy32 = M.evaluate(lx, ly, pad, patch, flags, SCALE, torch.float32)
    return loss, per_patch, gx, gy, _rel_l2(gx32, gx), _rel_l2(gy32, gy)


def _hip(case, ly_grad=False, upstream=None):
    from spcl_amd import functional as F_hip
    N, C, H, W, pad, patch, flags = CASES[case]
    lx, ly = _logits(N, C, H, W)
    x = lx.to(DEV).contiguous(memory_format=torch.channels_last).requires_grad_(True)
    y = ly.to(DEV).contiguous(memory_format=torch.channels_last).requires_grad_(ly_grad)
    fl = None if flags is None else torch.tensor(flags, dtype=torch.uint8, device=DEV)
    out = []
    loss = F_hip.iic_patch_loss(x, y, padding=pad, patch_size=patch, scale=SCALE, flags=fl, out=out)
    (loss if upstream is None else upstream * loss).backward()
    torch.cuda.synchronize()
    return loss.detach().cpu(), out[0].cpu(), out[1].cpu(), x.grad.cpu(), None if y.grad is None else y.grad.cpu()


@pytest.mark.parametrize("case", range(len(CASES)), ids=IDS)
def test_losses_and_lx_gradient_vs_float64(case):
    from spcl_amd import functional as F_hip
    N, C, H, W, pad, patch, flags = CASES[case]
    ref_loss, ref_patches, ref_gx, _, e32x, _ = _reference(case)
    loss, patches, flag, gx, gy = _hip(case)
    assert patches.shape == ref_patches.shape == (len(F_hip.iic_patch_starts(H, patch)) * len(F_hip.iic_patch_starts(W, patch)),)
    err = (patches.double() - ref_patches).abs()
    small = ref_patches.abs() < 1e-4
    rel = err / ref_patches.abs().clamp_min(1e-300)
    lerr = abs(float(loss) - float(ref_loss)) / abs(float(ref_loss))
    gerr = _rel_l2(gx, ref_gx)
    print(f"{len(patches)} patches ({int(small.sum())} below 1e-4), loss_P {float(ref_patches.min()):.3g} .. "
          f"{float(ref_patches.max()):.3g}: worst rel {float(rel[~small].max()) if bool((~small).any()) else 0.0:.2e}, "
          f"worst abs among the small {float(err[small].max()) if bool(small.any()) else 0.0:.2e}; loss rel {lerr:.2e}; "
          f"d lx rel L2 {gerr:.2e} (float32 oracle: {e32x:.2e})")
    assert bool(((rel <= 1e-5) | (small & (err <= 1e-9))).all()), (float(rel.max()), float(err.max()))
    assert lerr <= 1e-5, (float(loss), float(ref_loss))
    assert gerr <= max(1e-5, e32x), (gerr, e32x)
    assert int(flag[0]) == 0
    assert gy is None  # ly did not require grad


@pytest.mark.parametrize("case", range(len(CASES)), ids=IDS)
def test_ly_gradient_vs_float64_and_lx_gradient_unchanged(case):
    _, _, ref_gx, ref_gy, _, e32y = _reference(case)
    loss0, patches0, _, gx0, _ = _hip(case)
    loss, patches, flag, gx, gy = _hip(case, ly_grad=True)
    gerr = _rel_l2(gy, ref_gy)
    print(f"d ly rel L2 {gerr:.2e} (float32 oracle: {e32y:.2e})")
    assert gerr <= max(1e-5, e32y), (gerr, e32y)
    assert torch.equal(gx, gx0) and torch.equal(loss, loss0) and torch.equal(patches, patches0)
    assert int(flag[0]) == 0


@pytest.mark.parametrize("case", range(len(CASES)), ids=IDS)
def test_a_second_call_gives_the_same_bits(case):
    a = _hip(case, ly_grad=True)
    b = _hip(case, ly_grad=True)
    for u, v in zip(a, b):
        assert torch.equal(u, v)


@pytest.mark.parametrize("case", range(len(CASES)), ids=IDS)
def test_non_unit_upstream_gradient(case):
    _, _, _, gx, gy = _hip(case, ly_grad=True)
    _, _, _, gx3, gy3 = _hip(case, ly_grad=True, upstream=3.0)
    assert _rel_l2(gx3, 3.0 * gx) <= 1e-6 and _rel_l2(gy3, 3.0 * gy) <= 1e-6, (_rel_l2(gx3, 3.0 * gx), _rel_l2(gy3, 3.0 * gy))


def test_module_on_probabilities_agrees_with_the_functional_on_logits():
    from spcl_amd import functional as F_hip
    from spcl_amd.contrastyou.losses.iic_loss import IIDSegmentationSmallPathLoss
    N, C, H, W, pad, patch, _ = CASES[1]
    lx, ly = _logits(N, C, H, W)
    x = lx.to(DEV).contiguous(memory_format=torch.channels_last)
    y = ly.to(DEV).contiguous(memory_format=torch.channels_last)
    crit = IIDSegmentationSmallPathLoss(padding=pad, patch_size=patch)
    assert repr(crit) == f"IIDSegmentationSmallPathLoss with patch_size=({patch}, {patch}) and padding={pad}."
    got = crit(x.softmax(1), y.softmax(1))
    want = F_hip.iic_patch_loss(x, y, padding=pad, patch_size=patch)
    also = crit.from_logits(x, y)
    crit.flush_check()
    ref, _ = M.loss(lx.double(), ly.double(), pad, patch)
    assert abs(float(got) - float(want)) <= 1e-5 * abs(float(want)), (float(got), float(want))
    assert torch.equal(also, want)
    assert abs(float(want) - float(ref)) <= 1e-5 * abs(float(ref)), (float(want), float(ref))


@pytest.mark.parametrize("shape", [CASES[3][:6], (2, 4, 33, 29, 1, 64)], ids=["case4", "33x29"])
def test_one_whole_map_patch_agrees_with_the_dense_criterion(shape):
    """patch_size >= max(H, W), no flags: the same arithmetic as functional.iic_loss(dense=True) with one subhead -- both
    add the joint exactly (fixed point) and run the criterion in float64"""
    from spcl_amd import functional as F_hip
    N, C, H, W, pad, patch = shape
    lx, ly = _logits(N, C, H, W)
    x = lx.to(DEV).contiguous(memory_format=torch.channels_last)
    y = ly.to(DEV).contiguous(memory_format=torch.channels_last)
    got = F_hip.iic_patch_loss(x, y, padding=pad, patch_size=patch)
    want = F_hip.iic_loss(x, y, num_subheads=1, num_clusters=C, padding=pad, dense=True)
    print(f"patch-wise {float(got):.9g}, dense {float(want):.9g}")
    assert abs(float(got) - float(want)) <= 1e-6 * abs(float(want)), (float(got), float(want))


@pytest.mark.parametrize("C,pad,patch,word", [(17, 1, 8, "C = 17"), (4, 8, 8, "padding 8"), (4, 1, 1, "patch size 1")])
def test_argument_errors_carry_the_librarys_message(C, pad, patch, word):
    from spcl_amd import functional as F_hip
    x = torch.zeros(1, C, 8, 8, device=DEV)
    with pytest.raises(RuntimeError, match=word):
        F_hip.iic_patch_loss(x, x, padding=pad, patch_size=patch)
