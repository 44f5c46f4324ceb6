"""Float64 CPU restatement of the IIC criteria (contrastyou/losses/iic_loss.py: IIDLoss, IIDSegmentationLoss, compute_joint)
and the consistency criterion (semi_seg/hooks/consistency.py), written as the reference writes them, for the tests of
csrc/iic.hip.  Flags follow spcl_flip_batch: bit 0 flips H, bit 1 flips W."""
import torch
import torch.nn.functional as F


def flip(x, flags):
    if flags is None:
        return x
    out = []
    for n in range(x.shape[0]):
        v, f = x[n], int(flags[n])
        if f & 1:
            v = v.flip(-2)
        if f & 2:
            v = v.flip(-1)
        out.append(v)
    return torch.stack(out, 0)


def grouped_softmax(logits, S, K):
    N, _, H, W = logits.shape
    return [logits[:, s * K:(s + 1) * K].softmax(1) for s in range(S)]


def joint_dense(px, py, padding):
    """J [T, T, K, K] of two [N, K, H, W] maps (the F.conv2d of iic_loss.py:78)"""
    x = px.permute(1, 0, 2, 3).contiguous()
    y = py.permute(1, 0, 2, 3).contiguous()
    return F.conv2d(x, weight=y, padding=(padding, padding)).permute(2, 3, 0, 1)


def iid_segmentation_loss(px, py, padding, lamda=1.0):
    """IIDSegmentationLoss.__call__ (iic_loss.py:62-100) without the simplex asserts"""
    k = px.shape[1]
    x = px.permute(1, 0, 2, 3).contiguous()
    y = py.permute(1, 0, 2, 3).contiguous()
    p_i_j = F.conv2d(x, weight=y, padding=(padding, padding))
    p_i_j = p_i_j - p_i_j.min().detach() + 1e-16
    T = padding * 2 + 1
    p_i_j = p_i_j.permute(2, 3, 0, 1)
    p_i_j = p_i_j / p_i_j.sum(dim=3, keepdim=True).sum(dim=2, keepdim=True)
    p_i_j = (p_i_j + p_i_j.permute(0, 1, 3, 2)) / 2.0
    p_i_mat = p_i_j.sum(dim=2, keepdim=True).repeat(1, 1, k, 1)
    p_j_mat = p_i_j.sum(dim=3, keepdim=True).repeat(1, 1, 1, k)
    return (-p_i_j * (torch.log(p_i_j + 1e-16) - lamda * torch.log(p_i_mat + 1e-16)
                      - lamda * torch.log(p_j_mat + 1e-16))).sum() / (T * T)


def dense_loss_from_joint(j):
    """the criterion of IIDSegmentationLoss from its raw joint [T, T, K, K]"""
    T, k = j.shape[0], j.shape[2]
    p = j - j.min().detach() + 1e-16
    p = p / p.sum(dim=3, keepdim=True).sum(dim=2, keepdim=True)
    p = (p + p.permute(0, 1, 3, 2)) / 2.0
    pi = p.sum(dim=2, keepdim=True).repeat(1, 1, k, 1)
    pj = p.sum(dim=3, keepdim=True).repeat(1, 1, 1, k)
    return (-p * (torch.log(p + 1e-16) - torch.log(pi + 1e-16) - torch.log(pj + 1e-16))).sum() / (T * T)


def compute_joint(x_out, x_tf_out, symmetric=True):
    p_i_j = (x_out.unsqueeze(2) * x_tf_out.unsqueeze(1)).sum(dim=0)
    if symmetric:
        p_i_j = (p_i_j + p_i_j.t()) / 2.0
    return p_i_j / p_i_j.sum()


def iid_loss(x_out, x_tf_out, lamb=1.0):
    """IIDLoss.forward (iic_loss.py:29-51) -> (loss, loss_no_lamb, p_i_j)"""
    _, k = x_out.size()
    p_i_j = compute_joint(x_out, x_tf_out)
    p_i = p_i_j.sum(dim=1).view(k, 1).expand(k, k)
    p_j = p_i_j.sum(dim=0).view(1, k).expand(k, k)
    loss = (-p_i_j * (torch.log(p_i_j + 1e-10) - lamb * torch.log(p_j + 1e-10) - lamb * torch.log(p_i + 1e-10))).sum()
    loss_no_lamb = (-p_i_j * (torch.log(p_i_j + 1e-10) - torch.log(p_j + 1e-10) - torch.log(p_i + 1e-10))).sum()
    return loss, loss_no_lamb, p_i_j


def iic_hook_loss(lx, ly, S, K, padding, dense, flags=None):
    """mean over subheads of the criterion on softmax(flip(lx)) / softmax(ly) (discretemi.py:98-103)"""
    px = grouped_softmax(flip(lx, flags), S, K)
    py = grouped_softmax(ly, S, K)
    if dense:
        return sum(iid_segmentation_loss(a, b, padding) for a, b in zip(px, py)) / S
    return sum(iid_loss(a.flatten(1), b.flatten(1))[0] for a, b in zip(px, py)) / S


def consistency(a, b, weight, flags=None):
    """consistency.py:30-35"""
    pa = flip(a, flags).softmax(1)
    pb = b.softmax(1)
    return weight * F.mse_loss(pa.detach(), pb)
