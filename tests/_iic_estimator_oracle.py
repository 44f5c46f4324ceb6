"""CPU restatements for the tests of the IIC estimators' kernels, built on tests/_iic_oracle.py and tests/_midl_oracle.py:

* ``patch_heads_*``: the decoder criterion of ``IICEstimator`` (semi_seg/mi_estimator/discrete_mi_estimator.py:53-60) on
  logits -- per subhead ``IIDSegmentationSmallPathLoss(padding, patch_size)`` on ``softmax(lx_s)`` / ``softmax(flip(ly)_s)``,
  summed over the subheads and scaled;
* ``group_l2norm_temp``: ``Normalize() if normalize else Identical()`` then ``SoftmaxWithT``'s division
  (contrastyou/projectors/heads.py:42-75, nn.py:29-36, :50-58), per subhead, on the logits;
* ``cluster_head_logits`` / ``dense_cluster_head_logits``: the heads up to (not including) the softmax, from a state dict
  with the reference's keys.

Everything runs in the dtype of its inputs (float64 for the reference, float32 for the reference's own arithmetic)."""
import torch
import torch.nn.functional as F

from tests import _midl_oracle as M


def patch_heads_losses(lx, ly, S, K, padding, patch, flags=None):
    """[S][nP] list of lists of loss_{s,P}; channels >= S*K of the maps are ignored"""
    return [M.patch_losses(lx[:, s * K:(s + 1) * K], ly[:, s * K:(s + 1) * K], padding, patch, flags) for s in range(S)]


def patch_heads_loss(lx, ly, S, K, padding, patch, flags=None, scale=1.0):
    per = patch_heads_losses(lx, ly, S, K, padding, patch, flags)
    return scale * sum(torch.stack(p).mean() for p in per), per


def patch_heads_evaluate(lx, ly, S, K, padding, patch, flags, scale, dtype):
    """-> (loss, losses [S, nP], d loss / d lx, d loss / d ly), detached, computed in ``dtype``"""
    x = lx.to(dtype).requires_grad_(True)
    y = ly.to(dtype).requires_grad_(True)
    total, per = patch_heads_loss(x, y, S, K, padding, patch, flags, scale)
    total.backward()
    return total.detach(), torch.stack([torch.stack(p) for p in per]).detach(), x.grad, y.grad


def group_l2norm_temp(l, S, K, normalize, T):
    """[..., >= S*K] rows (the subheads along the LAST axis) -> the first S*K columns, normalised per subhead and over T"""
    out = []
    for s in range(S):
        g = l[..., s * K:(s + 1) * K]
        if normalize:
            g = F.normalize(g, p=2, dim=-1)
        out.append(g / T)
    return torch.cat(out, -1)


def _sub(sd, prefix, s, idx, name):
    return sd[f"{prefix}{s}.{idx}.{name}"]


def cluster_head_logits(feat, sd, S, head_type, normalize, T, prefix="_headers."):
    """ClusterHead (heads.py:124-145) without the final softmax: [N, S*K] rows"""
    x = feat.mean((2, 3))
    out = []
    for s in range(S):
        if head_type == "mlp":
            h = F.leaky_relu(F.linear(x, _sub(sd, prefix, s, 2, "weight"), _sub(sd, prefix, s, 2, "bias")), 0.01)
            o = F.linear(h, _sub(sd, prefix, s, 4, "weight"), _sub(sd, prefix, s, 4, "bias"))
        else:
            o = F.linear(x, _sub(sd, prefix, s, 2, "weight"), _sub(sd, prefix, s, 2, "bias"))
        out.append((F.normalize(o, p=2, dim=1) if normalize else o) / T)
    return torch.cat(out, 1)


def dense_cluster_head_logits(feat, sd, S, head_type, normalize, T, prefix="_headers."):
    """DenseClusterHead (heads.py:149-169) without the final softmax: [N, S*K, H, W]"""
    out = []
    for s in range(S):
        if head_type == "mlp":
            h = F.leaky_relu(F.conv2d(feat, _sub(sd, prefix, s, 0, "weight"), _sub(sd, prefix, s, 0, "bias")), 0.01)
            o = F.conv2d(h, _sub(sd, prefix, s, 2, "weight"), _sub(sd, prefix, s, 2, "bias"))
        else:
            o = F.conv2d(feat, _sub(sd, prefix, s, 0, "weight"), _sub(sd, prefix, s, 0, "bias"))
        out.append((F.normalize(o, p=2, dim=1) if normalize else o) / T)
    return torch.cat(out, 1)


# ---------------------------------------------------------------------------------------------- the recorded reference
def load_golden(path):
    """tests/golden/g15_iic_estimator.npz (tools/gen_golden_iic_estimator.py) -> (head case keys, estimator case keys, dict
    of tensors; the ``/keys`` entries stay lists of names)"""
    import numpy as np
    z = np.load(path)
    data = {k: ([str(n) for n in z[k]] if k.endswith("/keys") or k.endswith("_cases") else torch.from_numpy(z[k]))
            for k in z.files}
    return data["head_cases"], data["estimator_cases"], data


def parse_case(key):
    """'head/dense_mlp_n1_t0.5' / 'estimator/Up_conv3_linear_n0_t1.0' -> (dense or layer name, head_type, normalize, T)"""
    kind, rest = key.split("/")
    *name, head_type, nz, t = rest.split("_")
    name = "_".join(name)
    return (name == "dense" if kind == "head" else name), head_type, bool(int(nz[1:])), float(t[1:])


def golden_state(data, key):
    return {k: data[f"{key}/init/{k}"] for k in data[key + "/keys"]}


def head_probs(feat, sd, dense, S, K, head_type, normalize, T):
    """[S, N, K(, H, W)] probability maps of a head, as the fixture stacks the reference's list"""
    lg = (dense_cluster_head_logits if dense else cluster_head_logits)(feat, sd, S, head_type, normalize, T)
    return torch.stack([lg[:, s * K:(s + 1) * K].softmax(1) for s in range(S)], 0)


def estimator_forward(feat1, feat2, sd, dense, S, K, head_type, normalize, T, padding, patch):
    """``IICEstimator.forward(feat1, feat2)`` (discrete_mi_estimator.py:53-65): heads on cat([feat1, feat2]), then the mean
    over subheads of IIDLoss / IIDSegmentationSmallPathLoss on the two halves.  ``sd`` has the keys of the HEAD."""
    from tests._iic_oracle import iid_loss
    n = feat1.shape[0]
    lg = (dense_cluster_head_logits if dense else cluster_head_logits)(torch.cat([feat1, feat2], 0), sd, S, head_type,
                                                                       normalize, T)
    if dense:
        return patch_heads_loss(lg[:n], lg[n:], S, K, padding, patch, None, 1.0 / S)[0]
    return sum(iid_loss(lg[:n, s * K:(s + 1) * K].softmax(1), lg[n:, s * K:(s + 1) * K].softmax(1))[0] for s in range(S)) / S
