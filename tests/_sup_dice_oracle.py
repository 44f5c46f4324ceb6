"""Float64 torch restatement of the soft-Dice + class-weighted KL criterion (contrastyou/losses/dice.py),
differentiated by autograd.  CPU only; nothing of the package is imported."""
import torch


def one_hot(labels: torch.Tensor, C: int) -> torch.Tensor:
    """[N,H,W] integer labels -> [N,C,H,W] float64; a label outside [0, C) gives an all-zero row"""
    classes = torch.arange(C, device=labels.device).view(1, C, 1, 1)
    return (labels.unsqueeze(1) == classes).double()


def dice_kl(logits: torch.Tensor, labels: torch.Tensor, *, dice_weight=1.0, kl_weight=1.0, class_weight=None,
            include_background=True, per_sample=False, smooth=1e-5, eps=1e-16):
    """-> (loss, L_kl, L_dice) in float64 on the float32 logits as given"""
    x = logits.double()
    N, C, H, W = x.shape
    p = x.softmax(1)
    t = one_hot(labels, C)
    w = torch.ones(C, dtype=torch.float64) if class_weight is None else torch.as_tensor(class_weight, dtype=torch.float64)
    dims = (2, 3) if per_sample else (0, 2, 3)
    inter, psum, tsum = (p * t).sum(dims), p.sum(dims), t.sum(dims)
    ratio = (2 * inter + smooth) / (psum + tsum + smooth)
    ratio = ratio.reshape(-1, C)[:, (0 if include_background else 1):]
    l_dice = 1 - ratio.mean()
    # sum_c -t_c w_c log((p_c + eps) / (1 + eps)): only the labelled class has t_c != 0
    l_kl = (-(t * w.view(1, C, 1, 1).to(x.device) * torch.log((p + eps) / (1 + eps))).sum(1)).mean()
    return dice_weight * l_dice + kl_weight * l_kl, l_kl, l_dice


def dice_kl_with_grad(logits: torch.Tensor, labels: torch.Tensor, **kw):
    """-> (loss, d loss / d logits, L_kl, L_dice), all float64"""
    x = logits.detach().double().requires_grad_(True)
    loss, l_kl, l_dice = dice_kl(x, labels, **kw)
    (g,) = torch.autograd.grad(loss, x)
    return loss.detach(), g, l_kl.detach(), l_dice.detach()


def kl_div_onehot(logits: torch.Tensor, labels: torch.Tensor, eps=1e-16):
    """``KL_div(eps)(softmax(logits), one_hot(labels))`` restated: mean over pixels of sum_c -t log((p + eps) / (t + eps))"""
    p = logits.double().softmax(1)
    t = one_hot(labels, p.shape[1])
    return (-t * torch.log((p + eps) / (t + eps))).sum(1).mean()


def dice_counts(pred: torch.Tensor, labels: torch.Tensor, C: int):
    """(inter, union) [N, C] int64 of two class-coded maps, as ``functional.dice_counts``"""
    a, b = one_hot(pred, C), one_hot(labels, C)
    return (a * b).sum((2, 3)).long(), (a.sum((2, 3)) + b.sum((2, 3))).long()
