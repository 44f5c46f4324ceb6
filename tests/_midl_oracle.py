"""CPU restatement of ``IIDSegmentationSmallPathLoss`` (contrastyou/losses/iic_loss.py:103-128 with ``patch_generator``
:154-162) on logits, for the tests of csrc/iic_patch.hip: per patch, ``iid_segmentation_loss`` of tests/_iic_oracle.py on the
crops of ``softmax(lx)`` and ``softmax(flip(ly))``, then the mean.  The start lists are computed here from the formula,
independently of ``functional.iic_patch_starts``.  It runs in the dtype of its inputs (float64 for the reference, float32 for
the reference's own arithmetic)."""
import torch

from tests._iic_oracle import flip, iid_segmentation_loss


def starts(h, patch):
    """0, s, 2s, ... < h - patch, then max(h - patch, 0); s = patch // 2"""
    s, out, k = patch // 2, [], 0
    while k < h - patch:
        out.append(k)
        k += s
    return out + [max(h - patch, 0)]


def patch_losses(lx, ly, padding, patch, flags=None):
    """the list of loss_P, patches in row-major order of their (row start, column start)"""
    px, py = lx.softmax(1), flip(ly, flags).softmax(1)
    H, W = px.shape[2:]
    return [iid_segmentation_loss(px[:, :, a:min(a + patch, H), b:min(b + patch, W)],
                                  py[:, :, a:min(a + patch, H), b:min(b + patch, W)], padding)
            for a in starts(H, patch) for b in starts(W, patch)]


def loss(lx, ly, padding, patch, flags=None, scale=1.0):
    per_patch = patch_losses(lx, ly, padding, patch, flags)
    return scale * torch.stack(per_patch).mean(), per_patch


def evaluate(lx, ly, padding, patch, flags, scale, dtype):
    """-> (loss, per-patch losses [nP], d loss / d lx, d loss / d ly), all detached, computed in ``dtype``"""
    x = lx.to(dtype).requires_grad_(True)
    y = ly.to(dtype).requires_grad_(True)
    total, per_patch = loss(x, y, padding, patch, flags, scale)
    total.backward()
    return total.detach(), torch.stack(per_patch).detach(), x.grad, y.grad
