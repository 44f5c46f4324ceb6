"""Oracle of the boundary loss (contrastyou/losses/boundary.py, INTEGRATION.md "Boundary loss"): signed distance maps by
scipy's exact Euclidean distance transform, an integer brute force to hold scipy to, and a float64 autograd restatement of the
criterion with tests/_sup_dice_oracle.py's region term.  CPU only; nothing of the package is imported."""
import numpy as np
import torch
from scipy.ndimage import distance_transform_edt as edt

from tests import _sup_dice_oracle as R


def signed_distance_plane(m: np.ndarray) -> np.ndarray:
    """one boolean [H, W] membership map -> float64 phi: edt(~m) outside, -(edt(m) - 1) inside; zeros when m is empty or full
    (scipy would measure a full map against a corner outside the image)"""
    m = np.asarray(m, dtype=bool)
    if not m.any() or m.all():
        return np.zeros(m.shape, dtype=np.float64)
    return edt(~m) * ~m - (edt(m) - 1.0) * m


def signed_distance_ref(labels: torch.Tensor, classes) -> torch.Tensor:
    """[N,H,W] integer labels -> [N, |classes|, H, W] float32 (the float64 value rounded once)"""
    lab = labels.cpu().numpy()
    out = np.stack([np.stack([signed_distance_plane(lab[n] == c) for c in classes]) for n in range(lab.shape[0])])
    return torch.from_numpy(out.astype(np.float32))


def signed_distance_brute(m: np.ndarray) -> np.ndarray:
    """the definition itself: for every pixel the minimum, over ALL pixels of the opposite membership, of the integer
    (dy)^2 + (dx)^2, then one float64 square root and the sign rule"""
    m = np.asarray(m, dtype=bool)
    H, W = m.shape
    out = np.zeros((H, W), dtype=np.float64)
    if not m.any() or m.all():
        return out
    ys, xs = np.mgrid[0:H, 0:W]
    for inside in (False, True):
        qy, qx = np.nonzero(m == inside)          # the queries
        ty, tx = np.nonzero(m != inside)          # the opposite membership
        d2 = ((qy[:, None] - ty[None, :]).astype(np.int64) ** 2 + (qx[:, None] - tx[None, :]).astype(np.int64) ** 2).min(1)
        d = np.sqrt(d2.astype(np.float64))
        out[qy, qx] = -(d - 1.0) if inside else d
    return out + 0.0  # (-0.0 -> 0.0, as the subtraction in signed_distance_plane leaves it)


def boundary_terms(logits: torch.Tensor, phi: torch.Tensor, classes):
    """-> (L_B, A): the mean of p * phi over (n, listed class, pixel), and the mean of |p * phi| over the same terms"""
    p = logits.double().softmax(1)[:, list(classes)]
    t = p * phi.double()
    return t.mean(), t.abs().mean()


def boundary_loss(logits: torch.Tensor, labels: torch.Tensor, *, alpha, classes=None, **region):
    """-> (loss, L_region, L_B, A) in float64 on the float32 logits as given; ``region``: dice_kl's keywords"""
    C = logits.shape[1]
    classes = tuple(range(1, C)) if classes is None else tuple(classes)
    l_region, _, _ = R.dice_kl(logits, labels, **region)
    l_b, a = boundary_terms(logits, signed_distance_ref(labels, classes), classes)
    return l_region + float(alpha) * l_b, l_region, l_b, a


def boundary_loss_with_grad(logits: torch.Tensor, labels: torch.Tensor, **kw):
    """-> (loss, d loss / d logits, L_region, L_B, A), all float64"""
    x = logits.detach().double().requires_grad_(True)
    loss, l_region, l_b, a = boundary_loss(x, labels, **kw)
    (g,) = torch.autograd.grad(loss, x)
    return loss.detach(), g, l_region.detach(), l_b.detach(), a.detach()
